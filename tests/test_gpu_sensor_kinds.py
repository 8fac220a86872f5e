"""Extended builtin sensors on the GPU (csrc/sensor_ext.hip): every kind x object type x ref
pair of the probe robot (tests/sensor_probe.py) after forward(), step() and step(4) against the
fp64 reference (tests/sensor_ref.py) evaluated on the engine's own fields, at batch sizes 1 and
70 with per-world site / geom / inertial frames; the identities with the step kernels' gyro /
velocimeter / accelerometer; cutoffs; unit quaternions; step(4) == 4 x step(1) == graph replay;
the masked forward; and the G1 velocity env with six extended sensors added to its scene.

Bounds: a copy kind is bit for bit; a computed kind is within (n + 1) 2^-24 T, n the kind's
rounding count and T its term magnitude (tests/sensor_ref.py).  Measured largest
err / ((n + 1) 2^-24 T) per kind (MI355X, both batch sizes, all three calls; "+ref": with a
ref frame; the kinds not listed are copies, bit for bit):
  framepos+ref 0.29, framequat 0.41, framequat+ref 0.17, framexaxis+ref 0.46, frameyaxis+ref 0.37,
  framezaxis+ref 0.45, framelinvel 0.32, framelinvel+ref 0.14, frameangvel+ref 0.12,
  framelinacc 0.16
"""

import warnings

import numpy as np
import pytest
import torch

import sensor_probe as probe
import sensor_ref as ref
from parity_util import DATA_FIELDS

pytestmark = pytest.mark.gpu

FIELDS = ("xpos", "xquat", "xmat", "xipos", "ximat", "geom_xpos", "geom_xmat", "site_xpos",
          "site_xmat", "cvel", "cacc", "subtree_com", "subtree_linvel", "actuator_force",
          "actuator_length", "actuator_velocity", "qfrc_actuator")
STATE = ("qpos", "qvel", "qacc_warmstart", "time", "ctrl")
# R R^T - I of an fp32 rotation matrix formed from an fp32 quaternion product: the unit norm
# holds to a few 2^-24 after the product's 4 roundings, each entry of the matrix adds 3
N_ORTH = 16


def _make(n, device):
  from mjlab_amd.sim import MujocoCfg, Simulation, SimulationCfg
  m = probe.probe_model()
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")  # (the generic kernels: no specialisation for the probe)
    sim = Simulation(n, SimulationCfg(nconmax=16, njmax=64, specialize="never",
                                      mujoco=MujocoCfg(timestep=0.008, iterations=10, ls_iterations=20)),
                     m, device)
  # per-world local frames: site positions, geom and inertial orientations
  sim.expand_model_fields(("site_pos", "geom_quat", "body_iquat"))
  g = torch.Generator().manual_seed(n)
  sim.model.site_pos[:] += (0.02 * (torch.rand(sim.model.site_pos.shape, generator=g) - 0.5)).to(device)
  for f in ("geom_quat", "body_iquat"):
    q = getattr(sim.model, f)
    q[:] = torch.nn.functional.normalize(q + (0.2 * (torch.rand(q.shape, generator=g) - 0.5)).to(device), dim=-1)
  if n > 1:
    assert not torch.equal(sim.model.site_pos[0], sim.model.site_pos[1])
    assert not torch.equal(sim.model.geom_quat[0], sim.model.geom_quat[1])
    assert not torch.equal(sim.model.body_iquat[0], sim.model.body_iquat[1])
  q, v, ctrl = probe.random_states(m, n, seed=100 + n)
  sim.data.qpos[:] = torch.tensor(q, dtype=torch.float32, device=device)
  sim.data.qvel[:] = torch.tensor(v, dtype=torch.float32, device=device)
  sim.data.ctrl[:] = torch.tensor(ctrl, dtype=torch.float32, device=device)
  for _ in range(50):  # fall onto the plane: contacts and cacc are live
    sim.step()
  torch.cuda.synchronize()
  return m, sim


@pytest.fixture(scope="module", params=[1, 70])
def probe_sim(request, gpu_device):
  return _make(request.param, gpu_device)


def _arrays(m, sim):
  """The model arrays the reference reads: the compiled ones, the local frames and cutoffs
  as the engine holds them (fp32, per world)."""
  A = dict(m.arrays)
  for k in ("body_iquat", "geom_quat", "site_quat", "sensor_cutoff"):
    A[k] = getattr(sim.model, k).double().cpu().numpy()
  A["sensor_cutoff"] = A["sensor_cutoff"].reshape(-1, m.nsensor)[0]
  return A


def _reference(m, sim):
  d = {k: getattr(sim.data, k).double().cpu().numpy() for k in FIELDS}
  return ref.evaluate(_arrays(m, sim), d)


def _check(m, sim, what, ratios):
  torch.cuda.synchronize()
  got = sim.data.sensordata.cpu().numpy()
  val, T, n, own = _reference(m, sim)
  assert np.isfinite(got).all()
  for s, name in enumerate(m.names["sensor"]):
    st = int(m.sensor_type[s])
    if not ref.extended(st):
      continue
    a, k = int(m.sensor_adr[s]), int(m.sensor_dim[s])
    g, v, t, ns = got[:, a:a + k], val[:, a:a + k], T[:, a:a + k], int(n[a])
    if ns == 0:
      assert np.array_equal(g, v.astype(np.float32)), (what, name)
      continue
    bound = (ns + 1) * ref.EPS32 * t
    err = np.abs(g.astype(np.float64) - v)
    kind = ref.KIND_NAMES[st] + ("+ref" if m.sensor_reftype[s] else "")
    ratios[kind] = max(ratios.get(kind, 0.0), float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (what, name, float((err / np.maximum(bound, 1e-300)).max()))


def _entry(m, got, name):
  s = m.names["sensor"].index(name)
  a = int(m.sensor_adr[s])
  return got[:, a:a + int(m.sensor_dim[s])]


def test_every_kind_after_forward_step_and_four_substeps(probe_sim):
  m, sim = probe_sim
  ratios = {}
  sim.forward()
  _check(m, sim, "forward", ratios)
  sim.step()
  _check(m, sim, "step", ratios)
  sim.step(4)
  _check(m, sim, "step(4)", ratios)
  print("largest err / ((n + 1) 2^-24 T) per kind, batch", sim.num_envs,
        {k: round(v, 3) for k, v in sorted(ratios.items())})
  assert int(sim.data.ncon.max()) > 0  # the robot lies on the plane
  # the identities with the step kernels' site sensors, at the shared site
  got = sim.data.sensordata.double().cpu().numpy()
  _, T, n, _ = _reference(m, sim)
  imu = m.names["site"].index("imu")
  R = sim.data.site_xmat.double().cpu().numpy()[:, imu].reshape(-1, 3, 3)
  for sens, frame in (("gyro", "frameangvel_imu"), ("velocimeter", "framelinvel_imu"),
                      ("accelerometer", "framelinacc_imu")):
    s = m.names["sensor"].index(frame)
    t, nk = _entry(m, T, frame), int(n[int(m.sensor_adr[s])])
    tid = np.einsum("wij,wkj,wk->wi", np.abs(R), np.abs(R), t)
    want = np.einsum("wij,wj->wi", R, _entry(m, got, sens))
    bound = (2 * nk + 3 + N_ORTH + 2) * ref.EPS32 * tid
    assert (np.abs(_entry(m, got, frame) - want) <= bound).all(), (sens, frame)
  # framepos on a site without a ref is still the step kernels' own
  assert np.array_equal(_entry(m, got, "framepos_imu"), sim.data.site_xpos.double().cpu().numpy()[:, imu])


def test_cutoffs(probe_sim):
  m, sim = probe_sim
  sim.forward()
  torch.cuda.synchronize()
  got = sim.data.sensordata.cpu().numpy()
  cut = sim.model.sensor_cutoff.cpu().numpy().reshape(-1, m.nsensor)[0]
  c = lambda name: cut[m.names["sensor"].index(name)]
  # a gyro's cutoff, applied after the step kernel wrote it: the clamp of the uncut gyro
  gy = _entry(m, got, "gyro")
  assert np.array_equal(_entry(m, got, "gyro_cut"), np.clip(gy, -c("gyro_cut"), c("gyro_cut")))
  for name, plain in (("linvel_cut", "framelinvel_geom"), ("frc_cut", "actuatorfrc_hinge")):
    assert np.array_equal(_entry(m, got, name), np.clip(_entry(m, got, plain), -c(name), c(name))), name
  assert (np.abs(_entry(m, got, "pos_cut")) <= c("pos_cut")).all()
  # quaternions and axes ignore theirs
  assert np.array_equal(_entry(m, got, "quat_cut"), _entry(m, got, "framequat_body"))
  assert np.array_equal(_entry(m, got, "zaxis_cut"), _entry(m, got, "framezaxis_site"))
  # (the forearm's inertial frame is some 0.4 m from the base site: that cutoff always bites)
  assert (np.abs(_entry(m, got, "pos_cut")) == c("pos_cut")).any()


def test_framequat_entries_are_unit_quaternions(probe_sim):
  m, sim = probe_sim
  sim.data.sensordata.zero_()
  sim.step()
  torch.cuda.synchronize()
  got = sim.data.sensordata.double().cpu().numpy()
  val, T, n, _ = _reference(m, sim)
  nq = 0
  for s, name in enumerate(m.names["sensor"]):
    if int(m.sensor_type[s]) != ref.FRAMEQUAT:
      continue
    q, a = _entry(m, got, name), int(m.sensor_adr[s])
    # |q|^2 - 1: the inputs are unit to fp32 rounding, the product adds n roundings per entry
    assert (np.abs(np.sum(q * q, axis=1) - 1) <= 2 * (int(n[a]) + 4) * ref.EPS32 * 4).all(), name
    assert (np.abs(q - val[:, a:a + 4]) <= (int(n[a]) + 1) * ref.EPS32 * T[:, a:a + 4]).all(), name
    nq += 1
  assert nq >= 9


def _snap(sim, m):
  torch.cuda.synchronize()
  return sim.data.sensordata.clone()


def test_every_path_rounds_alike(probe_sim):
  """step(4) == four step(1) == a replayed capture of step(4), bit for bit; a masked forward
  leaves the unmasked worlds' entries alone."""
  m, sim = probe_sim
  d = sim.data
  state = {k: getattr(d, k).clone() for k in STATE}
  load = lambda: [getattr(d, k).copy_(v) for k, v in state.items()]
  own = torch.tensor(ref.evaluate(_arrays(m, sim), {k: getattr(d, k).double().cpu().numpy() for k in FIELDS})[3],
                     device=d.sensordata.device)
  sim.step(4)
  fused = _snap(sim, m)
  load()
  for _ in range(4):
    sim.step()
  single = _snap(sim, m)
  assert torch.equal(fused[:, own], single[:, own])
  load()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g, stream=s):
    sim.step(4)
  load()  # (capture does not run the step)
  d.sensordata.fill_(-7.0)
  g.replay()
  replay = _snap(sim, m)
  assert torch.equal(fused[:, own], replay[:, own])
  # masked forward: half the worlds (world 0 of a batch of one is masked out)
  n = sim.num_envs
  mask = (torch.arange(n, device=d.sensordata.device) % 2 == 1)
  d.sensordata.fill_(-7.0)
  sim.forward(mask)
  after = _snap(sim, m)
  assert (after[~mask][:, own] == -7.0).all()
  if n > 1:
    sim.forward()
    full = _snap(sim, m)
    assert torch.equal(after[mask][:, own], full[mask][:, own])


# ----------------------------------------------------------------------------------- G1 env
def _g1_env(device, extended_sensors):
  from mjlab_amd.envs import ManagerBasedRlEnv
  from mjlab_amd.envs import load_env_cfg
  cfg = probe.sensor_kinds_g1_cfg(64) if extended_sensors else load_env_cfg("Mjlab-Velocity-Flat-Unitree-G1")
  cfg.scene.num_envs = 64
  cfg.seed = 3
  cfg.sim.specialize = "always"  # (the build compiled the edited scene's kernels into the cache)
  env = ManagerBasedRlEnv(cfg, device=device)
  env.reset()
  return env


def _launches():
  import ctypes
  from mjlab_amd._lib import check, lib
  buf, one = (ctypes.c_int64 * 14)(), (ctypes.c_int64 * 1)()
  check(lib().mjx_launch_counts(buf, 14))
  check(lib().mjx_sensor_launch_count(one))
  return list(buf), int(one[0])


def test_g1_env_with_extended_sensors(gpu_device):
  """The G1 velocity env, fused and captured, with six extended sensors added through
  cfg.scene.sensors: the sensors do not touch what was there (every earlier sensordata entry
  and every data field, bit for bit, and the step kernels' launches), and cost one launch of
  their own per mjx_step."""
  from mjlab_amd._lib import check, lib
  outs = []
  for ext in (False, True):
    env = _g1_env(gpu_device, ext)
    info = env.sim.info()
    assert info["spec"] >= 1, info  # specialised kernels: compiled (shipped scene) or run-time
    env.enable_graph(capture=True, fused=True)
    assert env._fused is not None and getattr(env, "_fused_unsupported", None) is None
    g = torch.Generator(device=gpu_device).manual_seed(0)
    nact = env.action_manager.total_action_dim
    acts = [0.3 * (2 * torch.rand(64, nact, device=gpu_device, generator=g) - 1) for _ in range(4)]
    env.step(acts[0])  # records the graph
    torch.cuda.synchronize()
    check(lib().mjx_launch_counts_reset())
    # one uncaptured mjx_step for the launch counters (a captured launch counts once, at capture)
    env.sim.step(1)
    counts = _launches()
    for a in acts[1:]:
      env.step(a)
    torch.cuda.synchronize()
    outs.append((env.sim.mj_model, {k: getattr(env.sim.data, k).clone() for k in DATA_FIELDS}, counts))
  (m0, d0, (lc0, ns0)), (m1, d1, (lc1, ns1)) = outs
  assert m1.nsensor == m0.nsensor + 6 and m1.names["sensor"][:m0.nsensor] == m0.names["sensor"]
  assert lc0 == lc1 and sum(lc0) > 0
  assert ns0 == 0 and ns1 == 1
  for k in DATA_FIELDS:
    a, b = d0[k], d1[k]
    if k == "sensordata":
      b = b[:, :m0.nsensordata]
    assert torch.equal(a, b), k
  # and the new entries are what the reference makes of the env's own fields
  new = d1["sensordata"][:, m0.nsensordata:].double().cpu().numpy()
  A = dict(m1.arrays)  # (the local frames as the engine holds them: fp32)
  for k in ("body_iquat", "geom_quat", "site_quat"):
    A[k] = np.asarray(A[k], np.float32).astype(np.float64)
  val, T, n, own = ref.evaluate(A, {k: d1[k].double().cpu().numpy() for k in FIELDS})
  assert own[m0.nsensordata:].all() and not own[:m0.nsensordata].any()
  bound = (n + 1) * ref.EPS32 * T
  assert (np.abs(new - val[:, m0.nsensordata:]) <= bound[:, m0.nsensordata:]).all()
