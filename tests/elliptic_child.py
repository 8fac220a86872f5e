"""GPU child of tests/test_gpu_elliptic.py: runs the scenes of tests/elliptic_scenes.py on the
engine's generic kernels (`specialize="never"`, cone="elliptic"), every world with its own copy of
the scene's model fields, and writes what it computed, one npz per job part, for the parent to
compare with tests/elliptic_ref.py.

usage: elliptic_child.py <job.json> <out dir>; the job is {"scenes": [...], "batches": {scene: [n,
...]}, "plate": [n, ...], "overflow": [n, ...], "paths": [scene, [n, ...]], "sensor": scene,
"same": scene, "rollout": true}.

A part's file appears only once that part ran to the end, and the child stops at the first
error: the parent can tell which part faulted, and nothing runs on the GPU after a fault."""

from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "mjlab-1_amd"))

import elliptic_scenes as sc  # noqa: E402
from condim_child import FORWARD, STATS, STEP, _load, _report, _snapshot, _tile  # noqa: E402


def sim_cfg(m):
  from mjlab_amd.sim import MujocoCfg, SimulationCfg
  return SimulationCfg(nconmax=48, njmax=None, specialize="never",
                       mujoco=MujocoCfg(timestep=m.timestep, iterations=m.iterations, ls_iterations=m.ls_iterations,
                                        tolerance=m.tolerance, impratio=m.impratio, cone="elliptic"))


def _sim(name, n, expand=True, m=None, overflow=False):
  import dataclasses
  from mjlab_amd.sim import Simulation
  m = m if m is not None else sc.model(name)
  cfg = sim_cfg(m)
  if overflow:
    cfg = dataclasses.replace(cfg, engine_capacity=(16, 48))  # (njmax unset: a max capacity above)
  sim = Simulation(n, cfg, m, "cuda:0")
  if expand:
    f = sc.fields(name)
    sim.expand_model_fields(tuple(f))
    for k, v in f.items():
      t = getattr(sim.model, k)
      t[:] = torch.as_tensor(_tile(v, n), dtype=torch.float32).reshape(t.shape)
  return sim


def run_scene(name: str, n: int, m=None, overflow=False) -> dict:
  q, qv = (_tile(x, n) for x in sc.states(name))
  sim = _sim(name, n, m=m, overflow=overflow)
  info = sim.info()
  out = {"info": np.array([info[k] for k in ("spec", "spec_max", "nconmax", "njmax", "nconmax_max", "njmax_max")])}
  _load(sim, q, qv)
  sim.forward()
  torch.cuda.synchronize()
  for k in FORWARD + ("qacc", "contact_force", "solver_niter"):
    out["fwd_" + k] = getattr(sim.data, k).cpu().numpy()
  _load(sim, q, qv)
  sim.step()
  torch.cuda.synchronize()
  for k in STEP:
    out["step_" + k] = getattr(sim.data, k).cpu().numpy()
  st = sim.stats()
  out["stats"] = np.array([st[k] for k in STATS])
  return out


def run_plate(n: int, overflow: bool) -> dict:
  """The plate (24 contacts, 72 rows per world) in the default carve, or -- overflow -- in a fast
  carve of 16 contacts / 48 rows that every world exceeds: re-solved at max capacity."""
  return run_scene("plate", n, overflow=overflow)


def run_sensor(name: str) -> dict:
  """The scene with two contact sensors on the ball (found, force, torque): one slot reduced by
  mindist (the wave-cooperative form) and two slots unreduced (the serial form)."""
  from mjlab_amd.compiler.mjcf import parse_mjcf_string
  from mjlab_amd.compiler.model import ContactSensorSpec, EntitySpec, compile_scene
  base = sc.model(name)
  sens = [ContactSensorSpec("one", "geom", ["ball"], "geom", "floor", ("found", "force", "torque"), "mindist", 1),
          ContactSensorSpec("two", "geom", ["ball"], "geom", "floor", ("found", "force", "torque"), "none", 2)]
  m = compile_scene([EntitySpec(name="", xml=parse_mjcf_string(sc.scene_xml(name)))], terrain="none",
                    contact_sensors=sens, timestep=base.timestep, iterations=base.iterations,
                    ls_iterations=base.ls_iterations, tolerance=base.tolerance, impratio=base.impratio,
                    cone="elliptic")
  out = run_scene(name, sc.NWORLD, m=m)
  out["sensor_adr"] = np.asarray(m.arrays["sensor_adr"])
  out["sensor_dim"] = np.asarray(m.arrays["sensor_dim"])
  return out


def run_same(name: str) -> dict:
  """forward() and step() of the unexpanded sim and of one with the scene's fields expanded at
  the model's values: the fields that differ (parity_util.DATA_FIELDS and contact_torque)."""
  q, qv = sc.states(name)
  snaps = []
  for expand in (False, True):
    sim = _sim(name, sc.NWORLD, expand=False)
    if expand:
      sim.expand_model_fields(sc.FIELDS)
    s = {}
    for what in ("fwd", "step"):
      _load(sim, q, qv)
      sim.forward() if what == "fwd" else sim.step()
      torch.cuda.synchronize()
      s[what] = _snapshot(sim)
    snaps.append(s)
  rep = {what: _report(snaps[0][what], snaps[1][what]) for what in ("fwd", "step")}
  return {"same": np.array(json.dumps(rep)), "nefc_max": np.array(int(snaps[0]["step"]["nefc"].max())),
          "force_max": np.array(float(snaps[0]["step"]["contact_force"].abs().max()))}


def run_paths(name: str, n: int) -> dict:
  """step(4) against four step(1) and against a captured and replayed step(4)."""
  q, qv = (_tile(x, n) for x in sc.states(name))
  sim = _sim(name, n)
  snaps = {}
  _load(sim, q, qv)
  for _ in range(4):
    sim.step()
  torch.cuda.synchronize()
  snaps["single"] = _snapshot(sim)
  _load(sim, q, qv)
  sim.step(nsubstep=4)
  torch.cuda.synchronize()
  snaps["fused"] = _snapshot(sim)
  g = torch.cuda.CUDAGraph()
  side = torch.cuda.Stream()
  # warm the launch path outside capture, from the same state (engine counters are running maxima)
  _load(sim, q, qv)
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    sim.step(nsubstep=4)
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  _load(sim, q, qv)
  with torch.cuda.graph(g):
    sim.step(nsubstep=4)
  _load(sim, q, qv)
  g.replay()
  torch.cuda.synchronize()
  snaps["graph"] = _snapshot(sim)
  rep = {k: _report(snaps["fused"], snaps[k]) for k in ("single", "graph")}
  return {"paths": np.array(json.dumps(rep)), "nefc_max": np.array(int(snaps["fused"]["nefc"].max())),
          "moved": np.array(float((snaps["fused"]["qpos"].cpu() - torch.as_tensor(q, dtype=torch.float32)).abs().max()))}


def run_rollout() -> dict:
  """ROLLOUT_STEPS steps of the sliding puck: the state, the contact frame and force per step."""
  q, qv, _ = sc.rollout_start()
  sim = _sim("rollout", 1, expand=False)
  _load(sim, q[None], qv[None])
  n = sc.ROLLOUT_STEPS
  qs, vs = torch.zeros(n, 3, device="cuda:0"), torch.zeros(n, 3, device="cuda:0")
  fs, fr = torch.zeros(n, 3, device="cuda:0"), torch.zeros(n, 9, device="cuda:0")
  nc = torch.zeros(n, dtype=torch.int32, device="cuda:0")
  for k in range(n):
    sim.step()
    qs[k], vs[k] = sim.data.qpos[0], sim.data.qvel[0]
    fs[k], fr[k], nc[k] = sim.data.contact_force[0, 0], sim.data.contact_frame[0, 0].reshape(-1), sim.data.ncon[0]
  torch.cuda.synchronize()
  return {"qpos": qs.cpu().numpy(), "qvel": vs.cpu().numpy(), "force": fs.cpu().numpy(), "frame": fr.cpu().numpy(),
          "ncon": nc.cpu().numpy()}


def main() -> int:
  from mjlab_amd.sim.sim import GenericKernelWarning
  warnings.simplefilter("ignore", GenericKernelWarning)  # the generic kernels are the subject
  with open(sys.argv[1]) as fh:
    job = json.load(fh)
  outdir = sys.argv[2]

  def save(tag, out):
    tmp = os.path.join(outdir, f".{tag}.npz")
    np.savez(tmp, **out)
    os.replace(tmp, os.path.join(outdir, f"{tag}.npz"))
    print("ran", tag, flush=True)

  for name in job.get("scenes", []):
    for n in job.get("batches", {}).get(name, [sc.NWORLD]):
      save(f"{name}_{n}", run_scene(name, int(n)))
  for n in job.get("plate", []):
    save(f"plate_{n}", run_plate(int(n), False))
  for n in job.get("overflow", []):
    save(f"overflow_{n}", run_plate(int(n), True))
  if job.get("paths"):
    for n in job["paths"][1]:
      save(f"paths_{n}", run_paths(job["paths"][0], int(n)))
  if job.get("sensor"):
    save("sensor", run_sensor(job["sensor"]))
  if job.get("same"):
    save("same", run_same(job["same"]))
  if job.get("rollout"):
    save("rollout", run_rollout())
  return 0


if __name__ == "__main__":
  sys.exit(main())
