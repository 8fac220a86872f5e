"""GPU child of tests/test_gpu_model_zoo.py: runs zoo models (tests/model_zoo.py) on the engine
and writes what it computed, one npz per model, for the parent to compare with the fp64 oracle.

usage: zoo_child.py <job.json> <out dir>; the job is {"models": [...], "specialize": "never" |
"auto", "fused": [...models whose 4-substep step is compared with four single steps]}.

A model's file appears only once that model ran to the end, and the child stops at the first
error: the parent can tell which model faulted, and nothing runs on the GPU after a fault."""

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

import model_zoo as zoo  # noqa: E402
from parity_util import diff_detail, differing_outputs, output_snapshot  # noqa: E402

FORWARD = ("xpos", "xquat", "xipos", "subtree_com", "cvel", "qfrc_bias", "qfrc_passive",
           "actuator_force", "qacc_smooth", "sensordata", "ncon", "nefc")
STEP = ("qacc", "qvel", "qpos", "sensordata", "solver_niter", "ncon", "nefc", "contact_dist")


def _load(sim, q, qv, ctrl):
  d = sim.data
  d.qpos[:] = torch.as_tensor(q, dtype=torch.float32)
  d.qvel[:] = torch.as_tensor(qv, dtype=torch.float32)
  d.ctrl[:] = torch.as_tensor(ctrl, dtype=torch.float32)
  d.qacc_warmstart[:] = 0
  d.time[:] = 0


def run_model(name: str, specialize: str, fused: bool) -> dict:
  from mjlab_amd.sim import Simulation
  zm = zoo.get(name)
  m = zm.model
  q, qv, ctrl = zm.states()
  sim = Simulation(q.shape[0], zoo.sim_cfg(m, specialize), m, "cuda:0")
  out = {"info": np.array([sim.info()[k] for k in ("spec", "spec_max", "nconmax", "njmax")])}
  _load(sim, q, qv, ctrl)
  sim.forward()
  torch.cuda.synchronize()
  for k in FORWARD:
    out["fwd_" + k] = getattr(sim.data, k).cpu().numpy()
  out["fwd_qM"] = sim.mass_matrix().cpu().numpy()
  _load(sim, q, qv, ctrl)
  sim.step()
  torch.cuda.synchronize()
  for k in STEP:
    out["step_" + k] = getattr(sim.data, k).cpu().numpy()
  if fused:
    _load(sim, q, qv, ctrl)
    for _ in range(4):
      sim.step()
    torch.cuda.synchronize()
    single = output_snapshot(sim)
    _load(sim, q, qv, ctrl)
    sim.step(4)
    torch.cuda.synchronize()
    four = output_snapshot(sim)
    bad = differing_outputs(single, four)
    out["fused_bad"] = np.array(json.dumps({"fields": bad, "detail": diff_detail(single, four, bad)}))
  return out


def main() -> int:
  from mjlab_amd.sim.sim import GenericKernelWarning
  warnings.simplefilter("ignore", GenericKernelWarning)  # the generic kernels are the subject
  with open(sys.argv[1]) as fh:
    job = json.load(fh)
  outdir = sys.argv[2]
  for name in job["models"]:
    out = run_model(name, job.get("specialize", "never"), name in job.get("fused", []))
    tmp = os.path.join(outdir, f".{name}.npz")
    np.savez(tmp, **out)
    os.replace(tmp, os.path.join(outdir, f"{name}.npz"))
    print("ran", name, flush=True)
  return 0


if __name__ == "__main__":
  sys.exit(main())
