"""GPU child of tests/test_gpu_condim.py: runs the probe scenes of tests/condim_scenes.py on the
engine's generic kernels (`specialize="never"`), every world with its own copy of the scene's
model fields, and writes what it computed, one npz per job part, for the parent to compare with
tests/condim_ref.py.

usage: condim_child.py <job.json> <out dir>; the job is {"scenes": [...], "batches": {scene: [n,
...]}, "paths": [scene, [n, ...]], "sensor": scene, "same": scene, "rollout": true}.

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

import condim_scenes as sc  # noqa: E402
from parity_util import diff_detail, differing_outputs, output_snapshot  # noqa: E402

FORWARD = ("ncon", "nefc", "contact_dist")
STEP = ("qacc", "qvel", "qpos", "qfrc_constraint", "contact_force", "contact_torque", "contact_dist",
        "contact_pos", "contact_frame", "contact_geom", "ncon", "nefc", "solver_niter", "sensordata")
STATS = ("max_ncon", "max_nefc", "con_overflow", "row_overflow", "unsupported", "resolved")


def sim_cfg(m):
  from mjlab_amd.sim import MujocoCfg, SimulationCfg
  # (njmax unset: the capacities count the model's 2 (max_condim - 1) rows per contact)
  return SimulationCfg(nconmax=48, njmax=None, specialize="never",
                       mujoco=MujocoCfg(timestep=m.timestep, iterations=m.iterations, ls_iterations=m.ls_iterations,
                                        tolerance=m.tolerance, impratio=m.impratio))


def _load(sim, q, qv):
  d = sim.data
  d.qpos[:] = torch.as_tensor(q, dtype=torch.float32)
  d.qvel[:] = torch.as_tensor(qv, dtype=torch.float32)
  d.qacc_warmstart[:] = 0
  d.time[:] = 0


def _tile(x, n):
  return x[np.arange(n) % sc.NWORLD]


def _sim(name, n, expand=True, m=None):
  from mjlab_amd.sim import Simulation
  m = m if m is not None else sc.model(name)
  sim = Simulation(n, sim_cfg(m), m, "cuda:0")
  if expand:
    f = sc.fields(name)
    sim.expand_model_fields(tuple(f))
    for k, v in f.items():
      t = getattr(sim.model, k)
      t[:] = torch.as_tensor(_tile(v, n), dtype=torch.float32).reshape(t.shape)
  return sim


def _snapshot(sim):
  out = output_snapshot(sim)
  out["contact_torque"] = sim.data.contact_torque.clone()
  return out


def run_scene(name: str, n: int, m=None) -> dict:
  q, qv = (_tile(x, n) for x in sc.states(name))
  sim = _sim(name, n, m=m)
  info = sim.info()
  out = {"info": np.array([info[k] for k in ("spec", "spec_max", "nconmax", "njmax", "nconmax_max", "njmax_max")])}
  _load(sim, q, qv)
  sim.forward()
  torch.cuda.synchronize()
  for k in FORWARD:
    out["fwd_" + k] = getattr(sim.data, k).cpu().numpy()
  _load(sim, q, qv)
  sim.step()
  torch.cuda.synchronize()
  for k in STEP:
    out["step_" + k] = getattr(sim.data, k).cpu().numpy()
  st = sim.stats()
  out["stats"] = np.array([st[k] for k in STATS])
  # reset clears the torque like the force
  sim.reset()
  torch.cuda.synchronize()
  out["reset_wrench_max"] = np.array([float(sim.data.contact_force.abs().max()), float(sim.data.contact_torque.abs().max())])
  return out


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
                    ls_iterations=base.ls_iterations, tolerance=base.tolerance, impratio=base.impratio)
  out = run_scene(name, sc.NWORLD, m=m)
  out["sensor_adr"] = np.asarray(m.arrays["sensor_adr"])
  out["sensor_dim"] = np.asarray(m.arrays["sensor_dim"])
  return out


def _report(a: dict, b: dict) -> dict:
  bad = differing_outputs(a, b)
  return {"fields": bad, "detail": diff_detail(a, b, bad)}


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
          "torque_max": np.array(float(snaps[0]["step"]["contact_torque"].abs().max()))}


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
  # warm the launch path outside capture, from the same state: engine_counters [0, 1, 5] are
  # running maxima, and a warm-up from the evolved state could raise them past this rollout's
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
  """ROLLOUT_STEPS steps of the spinning ball with condim 3 and 4: the state after every step."""
  q, qv = sc.spin_down_start()
  out = {}
  for name in ("spin_down3", "spin_down4"):
    sim = _sim(name, 1, expand=False)
    _load(sim, q[None], qv[None])
    qs = torch.zeros(sc.ROLLOUT_STEPS, 7, device="cuda:0")
    vs = torch.zeros(sc.ROLLOUT_STEPS, 6, device="cuda:0")
    for k in range(sc.ROLLOUT_STEPS):
      sim.step()
      qs[k], vs[k] = sim.data.qpos[0], sim.data.qvel[0]
    torch.cuda.synchronize()
    out[name + "_qpos"], out[name + "_qvel"] = qs.cpu().numpy(), vs.cpu().numpy()
    out[name + "_unsupported"] = np.array(sim.stats()["unsupported"])
  return out


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
