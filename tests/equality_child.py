"""GPU child of tests/test_gpu_equality.py: runs the scenes of tests/equality_scenes.py on the
engine's generic kernels and writes what it computed for the parent to compare with the fp64
references.

usage: equality_child.py <job.json> <out dir>; the job is {"scenes": [...], "batches": [...],
"same": name, "paths": name, "rollout": name}:

  <scene>_<n>.npz  forward() and step() of the scene's first n worlds (fwd_* / step_* fields)
  same.npz         `same` with eq_data / eq_solref / eq_solimp expanded but left at the model's
                   values against the unexpanded sim, bit for bit (parity_util.DATA_FIELDS)
  paths.npz        `paths`: step(4), four step(1) and a replayed graph of step(4), bit for bit
  rollout.npz      `rollout`: equality_scenes.ROLLOUT_STEPS steps of world 2 under rollout_ctrl:
                   the largest |q_l + q_r| and the last state

A file appears only once its part ran to the end, and the child stops at the first error: the
parent can tell which part faulted, and nothing runs on the GPU after a fault."""

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

import equality_scenes as es  # noqa: E402
from parity_util import diff_detail, differing_outputs, output_snapshot  # noqa: E402

FORWARD = ("ncon", "nefc")
STEP = ("qacc", "qvel", "qpos", "qfrc_constraint", "contact_force", "contact_dist", "contact_frame", "ncon",
        "nefc", "solver_niter")


def sim_cfg(m):
  from mjlab_amd.sim import MujocoCfg, SimulationCfg
  return SimulationCfg(nconmax=48, njmax=160, specialize="never",
                       mujoco=MujocoCfg(timestep=m.timestep, iterations=m.iterations, ls_iterations=m.ls_iterations,
                                        tolerance=m.tolerance, impratio=m.impratio))


def _load(sim, q, qv, ctrl):
  d = sim.data
  d.qpos[:] = torch.as_tensor(q, dtype=torch.float32)
  d.qvel[:] = torch.as_tensor(qv, dtype=torch.float32)
  if ctrl.shape[1]:
    d.ctrl[:] = torch.as_tensor(ctrl, dtype=torch.float32)
  d.qacc_warmstart[:] = 0
  d.time[:] = 0


def _sim(name, n, expand=True):
  from mjlab_amd.sim import Simulation
  m = es.model(name)
  sim = Simulation(n, sim_cfg(m), m, "cuda:0")
  f = es.fields(name)
  if f and expand:
    sim.expand_model_fields(tuple(f))
    for k, v in f.items():
      t = getattr(sim.model, k)
      t[:] = torch.as_tensor(v[:n], dtype=torch.float32).reshape(t.shape)
  return sim


def run_scene(name: str, n: int) -> dict:
  q, qv, ctrl = (x[:n] for x in es.states(name))
  sim = _sim(name, n)
  out = {"info": np.array([sim.info()[k] for k in ("spec", "spec_max", "nconmax", "njmax")])}
  _load(sim, q, qv, ctrl)
  sim.forward()
  torch.cuda.synchronize()
  for k in FORWARD:
    out["fwd_" + k] = getattr(sim.data, k).cpu().numpy()
  _load(sim, q, qv, ctrl)
  sim.step()
  torch.cuda.synchronize()
  for k in STEP:
    out["step_" + k] = getattr(sim.data, k).cpu().numpy()
  return out


def _report(a: dict, b: dict) -> dict:
  bad = differing_outputs(a, b)
  return {"fields": bad, "detail": diff_detail(a, b, bad)}


def run_same(name: str) -> dict:
  """forward() and step() of the unexpanded sim and of one with the three eq_* float fields
  expanded at the model's values: the fields that differ."""
  q, qv, ctrl = es.states(name)
  snaps = []
  for expand in (False, True):
    sim = _sim(name, es.NWORLD, expand=False)
    if expand:
      sim.expand_model_fields(es.EQ_FIELDS)
    s = {}
    for what in ("fwd", "step"):
      _load(sim, q, qv, ctrl)
      sim.forward() if what == "fwd" else sim.step()
      torch.cuda.synchronize()
      s[what] = output_snapshot(sim)
    snaps.append(s)
  rep = {what: _report(snaps[0][what], snaps[1][what]) for what in ("fwd", "step")}
  return {"same": np.array(json.dumps(rep)), "nefc_min": np.array(int(snaps[0]["step"]["nefc"].min()))}


def run_paths(name: str) -> dict:
  """step(4) against four step(1) and against a captured and replayed step(4)."""
  q, qv, ctrl = es.states(name)
  sim = _sim(name, es.NWORLD)
  snaps = {}
  _load(sim, q, qv, ctrl)
  for _ in range(4):
    sim.step()
  torch.cuda.synchronize()
  snaps["single"] = output_snapshot(sim)
  _load(sim, q, qv, ctrl)
  sim.step(nsubstep=4)
  torch.cuda.synchronize()
  snaps["fused"] = output_snapshot(sim)
  g = torch.cuda.CUDAGraph()
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    sim.step(nsubstep=4)  # warm the launch path outside capture
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  _load(sim, q, qv, ctrl)
  with torch.cuda.graph(g):
    sim.step(nsubstep=4)
  _load(sim, q, qv, ctrl)
  g.replay()
  torch.cuda.synchronize()
  snaps["graph"] = output_snapshot(sim)
  rep = {k: _report(snaps["fused"], snaps[k]) for k in ("single", "graph")}
  return {"paths": np.array(json.dumps(rep)), "nefc_max": np.array(int(snaps["fused"]["nefc"].max())),
          "moved": np.array(float((snaps["fused"]["qpos"].cpu() - torch.as_tensor(q, dtype=torch.float32)).abs().max()))}


def run_rollout(name: str) -> dict:
  q, qv, ctrl = (x[2:3] for x in es.states(name))
  sim = _sim(name, 1)
  _load(sim, q, qv, ctrl)
  d = sim.data
  worst = torch.zeros(1, device=d.qpos.device)
  for k in range(es.ROLLOUT_STEPS):
    d.ctrl[:, 0] = float(es.rollout_ctrl(k))
    sim.step()
    worst = torch.maximum(worst, (d.qpos[:, 1] + d.qpos[:, 2]).abs())
  torch.cuda.synchronize()
  return {"worst": worst.cpu().numpy(), "qpos": d.qpos.cpu().numpy(), "qvel": d.qvel.cpu().numpy()}


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
    for n in job.get("batches", []):
      save(f"{name}_{n}", run_scene(name, int(n)))
  for key, fn in (("same", run_same), ("paths", run_paths), ("rollout", run_rollout)):
    if job.get(key):
      save(key, fn(job[key]))
  return 0


if __name__ == "__main__":
  sys.exit(main())
