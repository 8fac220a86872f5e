"""GPU child of tests/test_gpu_constraint_params.py: runs the probe scenes of
tests/constraint_scenes.py on the engine's generic kernels, every world with its own copy of
the scene's model fields, and writes what it computed, one npz per scene, for the parent to
compare with tests/constraint_ref.py and the fp64 oracle.

usage: constraint_child.py <job.json> <out dir>; the job is {"scenes": [...], "same": [...]}:
`same` names scenes (or zoo models) for which a sim with all of constraint_scenes.ALL_FIELDS
expanded but left at the model's values is compared bit for bit with the unexpanded sim.

A scene's file appears only once that scene ran to the end, and the child stops at the first
error: the parent can tell which scene faulted, and nothing runs on the GPU after a fault."""

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

import constraint_scenes as cs  # noqa: E402
from parity_util import diff_detail, differing_outputs, output_snapshot  # noqa: E402

FORWARD = ("ncon", "nefc", "contact_dist")
STEP = ("qacc", "qvel", "qpos", "qfrc_constraint", "contact_force", "contact_dist", "contact_pos",
        "contact_frame", "contact_geom", "ncon", "nefc", "solver_niter")


def sim_cfg(m):
  from mjlab_amd.sim import MujocoCfg, SimulationCfg
  return SimulationCfg(nconmax=48, njmax=160, specialize="never",
                       mujoco=MujocoCfg(timestep=m.timestep, iterations=m.iterations, ls_iterations=m.ls_iterations,
                                        tolerance=m.tolerance, impratio=m.impratio))


def _load(sim, q, qv, ctrl=None):
  d = sim.data
  d.qpos[:] = torch.as_tensor(q, dtype=torch.float32)
  d.qvel[:] = torch.as_tensor(qv, dtype=torch.float32)
  if ctrl is not None:
    d.ctrl[:] = torch.as_tensor(ctrl, dtype=torch.float32)
  d.qacc_warmstart[:] = 0
  d.time[:] = 0


def run_scene(name: str) -> dict:
  from mjlab_amd.sim import Simulation
  m = cs.model(name)
  q, qv = cs.states(name)
  sim = Simulation(cs.NWORLD, sim_cfg(m), m, "cuda:0")
  f = cs.fields(name)
  sim.expand_model_fields(tuple(f))
  for k, v in f.items():
    t = getattr(sim.model, k)
    t[:] = torch.as_tensor(v, dtype=torch.float32).reshape(t.shape)
  out = {"info": np.array([sim.info()[k] for k in ("spec", "spec_max", "nconmax", "njmax")])}
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
  return out


def run_same(name: str) -> dict:
  """forward() and step() of the unexpanded sim and of one with the ten fields expanded at the
  model's values: {"fwd": ..., "step": ...} of the fields that differ."""
  from mjlab_amd.sim import Simulation
  if name in cs.SCENES:
    m = cs.model(name)
    q, qv = cs.states(name)
    ctrl = None
  else:
    import model_zoo as zoo
    zm = zoo.get(name)
    m = zm.model
    q, qv, ctrl = zm.states()
  snaps = []
  for expand in (False, True):
    sim = Simulation(q.shape[0], sim_cfg(m), m, "cuda:0")
    if expand:
      sim.expand_model_fields(cs.ALL_FIELDS)
    s = {}
    for what in ("fwd", "step"):
      _load(sim, q, qv, ctrl)
      sim.forward() if what == "fwd" else sim.step()
      torch.cuda.synchronize()
      s[what] = output_snapshot(sim)
    snaps.append(s)
  rep = {}
  for what in ("fwd", "step"):
    bad = differing_outputs(snaps[0][what], snaps[1][what])
    rep[what] = {"fields": bad, "detail": diff_detail(snaps[0][what], snaps[1][what], bad)}
  return {"same": np.array(json.dumps(rep)), "ncon_max": np.array(int(snaps[0]["step"]["ncon"].max()))}


def main() -> int:
  from mjlab_amd.sim.sim import GenericKernelWarning
  warnings.simplefilter("ignore", GenericKernelWarning)  # the generic kernels are the subject
  with open(sys.argv[1]) as fh:
    job = json.load(fh)
  outdir = sys.argv[2]
  for tag, names, fn in (("", job.get("scenes", []), run_scene), ("same_", job.get("same", []), run_same)):
    for name in names:
      out = fn(name)
      tmp = os.path.join(outdir, f".{tag}{name}.npz")
      np.savez(tmp, **out)
      os.replace(tmp, os.path.join(outdir, f"{tag}{name}.npz"))
      print("ran", tag + name, flush=True)
  return 0


if __name__ == "__main__":
  sys.exit(main())
