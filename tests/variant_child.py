"""Child runner of tests/test_gpu_kernel_variants.py (a plain script, not a test module).

  python tests/variant_child.py <job.json> <out.npz>

runs the scenarios the JSON job names in this fresh process and records every mjData output
after every stage.  The engine caches its MJX355_* launch knobs in function-local statics, so
one process runs one setting: the knobs reach this process through its environment, and the
parent compares the recordings of differently configured children bit for bit.

Job: {"scenarios": ["g1", ...], "graph": true | false}.  Per scenario the Simulation is
built, seeded states (numpy, host) are loaded, and after each stage all of
parity_util.DATA_FIELDS, engine_counters[:, [0, 1, 5]], the event counts and the launch
counts of the stage (mjx_launch_counts) are stored under "<scenario>.<stage>.<name>":

  step1, step2, step3   three single sim.step() calls
  fused4                the saved state restored, one sim.step(nsubstep=4)
  masked                every third world given a fresh seeded state, sim.forward(mask) over them
  graph4                (job["graph"]) the saved state restored, sim.step(nsubstep=4) captured
                        by torch.cuda.graph and replayed

plus "<scenario>.info" (sim.info() in INFO_KEYS order, then stats()["unsupported"]).
MJX355_JIT=0 is set here, so no child compiles anything.
"""

from __future__ import annotations

import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "mjlab-1_amd"), HERE):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import numpy as np

INFO_KEYS = ("nconmax", "njmax", "nconmax_max", "njmax_max", "spec", "spec_max", "resolve_list",
             "row_classes")
STATE = ("qpos", "qvel", "qacc_warmstart", "ctrl", "time")
NCODES = 14  # phase codes 0 .. 12 and the classify kernel (include/mjx355.h mjx_launch_counts)
MASK_EVERY = 3

# scenario -> (task whose shipped SimulationCfg it runs, scene, fast carve override, worlds,
# MJX355_ROW_CLASSES at Simulation creation or None for the automatic choice, MJX355_NO_SPEC
# there).  The (20, 80) carve has no compiled specialisation and gets no row class by default:
# g1_small runs the generic kernels in the fast carve (the range chain, as Go1) and the
# specialised ones in the max carve, as an engine_capacity override of a shipped robot does.
# g1_small_cls is the same model as one the engine has no specialisation for at all (generic
# kernels in both carves), with one row class forced, so that worlds listed for the re-solve
# also meet the class launches and the fast-carve masked forward's J-in-global Newton (code 9).
SMALL_CLASS_CAP = 44
SCENARIOS = {
  "g1": ("Mjlab-Velocity-Flat-Unitree-G1", "g1_velocity", None, 96, None, False),
  "g1_small": ("Mjlab-Velocity-Flat-Unitree-G1", "g1_velocity", (20, 80), 96, None, False),
  "g1_small_cls": ("Mjlab-Velocity-Flat-Unitree-G1", "g1_velocity", (20, 80), 96, str(SMALL_CLASS_CAP), True),
  "hfield": ("Mjlab-Jump-Hfield-Unitree-G1", "g1_jump_hfield", None, 64, None, False),
  "go1": ("Mjlab-Velocity-Flat-Unitree-Go1", "go1_velocity", None, 64, None, False),
}


def scenario_cfg(name):
  """(SimulationCfg, compiled model with the cfg's solver options applied, worlds)."""
  from mjlab_amd.envs import load_env_cfg
  from mjlab_amd.scenes import load_scene
  task, scene, small, n = SCENARIOS[name][:4]
  cfg = load_env_cfg(task).sim
  if small is not None:
    cfg.engine_capacity = small
  m = load_scene(scene)
  cfg.mujoco.apply(m)  # (what Simulation does: the oracle reads the same options)
  m.contact_maxmatch = int(cfg.contact_sensor_maxmatch)
  return cfg, m, n


def scenario_states(name, m, n, fresh=False):
  """The scenario's seeded (qpos, qvel, ctrl); `fresh`: the states the masked worlds get."""
  from parity_util import g1_states, hfield_states
  k = 100 if fresh else 0
  if name.startswith("g1"):
    return g1_states(m, n, seed=11 + k)
  if name == "hfield":
    return hfield_states(m, n, seed=4 + k, dz=(-0.04, 0.2))
  from test_gpu_parity import _go1_states
  return _go1_states(m, n, seed=3 + k)


def masked_worlds(n):
  return np.arange(n) % MASK_EVERY == 0


def _run_scenario(name, graph, out):
  import ctypes

  import torch
  from mjlab_amd._lib import check, lib
  from mjlab_amd.sim import Simulation
  from parity_util import DATA_FIELDS

  cfg, m, n = scenario_cfg(name)
  classes, no_spec = SCENARIOS[name][4:]
  env = {**({"MJX355_ROW_CLASSES": classes} if classes is not None else {}),
         **({"MJX355_NO_SPEC": "1"} if no_spec else {})}
  os.environ.update(env)  # (both are read when the Simulation is created)
  try:
    sim = Simulation(n, cfg, m, "cuda:0")
  finally:
    for k in env:
      del os.environ[k]
  d = sim.data
  L = lib()

  def counts():
    buf = (ctypes.c_int64 * NCODES)()
    check(L.mjx_launch_counts(buf, NCODES))
    return np.array(list(buf), dtype=np.int64)

  def record(stage):
    torch.cuda.synchronize()
    for k in DATA_FIELDS:
      out[f"{name}.{stage}.{k}"] = getattr(d, k).cpu().numpy().copy()
    out[f"{name}.{stage}.engine_counters[0,1,5]"] = sim.engine_counters[:, [0, 1, 5]].cpu().numpy().copy()
    out[f"{name}.{stage}.event_counts"] = sim.event_counts().cpu().numpy().copy()
    out[f"{name}.{stage}.launch_counts"] = counts()
    check(L.mjx_launch_counts_reset())

  def load(q, qv, ctrl, worlds=None):
    sel = np.arange(n) if worlds is None else np.nonzero(worlds)[0]
    idx = torch.as_tensor(sel, device=d.qpos.device)
    for dst, src in ((d.qpos, q), (d.qvel, qv), (d.ctrl, ctrl)):
      dst[idx] = torch.as_tensor(src[sel], dtype=torch.float32, device=dst.device)
    d.qacc_warmstart[idx] = 0

  load(*scenario_states(name, m, n))
  saved = {k: getattr(d, k).clone() for k in STATE}

  def restore():
    for k, v in saved.items():
      getattr(d, k).copy_(v)

  torch.cuda.synchronize()
  check(L.mjx_launch_counts_reset())
  for i in range(3):
    sim.step()
    record(f"step{i + 1}")
  restore()
  sim.step(nsubstep=4)
  record("fused4")
  mask = masked_worlds(n)
  load(*scenario_states(name, m, n, fresh=True), worlds=mask)
  sim.forward(torch.as_tensor(mask.astype(np.uint8), device=d.qpos.device))
  record("masked")
  if graph:
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      sim.step(nsubstep=4)  # warm the launch path outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    restore()
    check(L.mjx_launch_counts_reset())
    with torch.cuda.graph(g):
      sim.step(nsubstep=4)
    restore()
    g.replay()
    record("graph4")
  info = sim.info()
  out[f"{name}.info"] = np.array([info[k] for k in INFO_KEYS] + [sim.stats()["unsupported"]],
                                 dtype=np.int64)


def main(argv):
  os.environ["MJX355_JIT"] = "0"
  t0 = time.time()
  with open(argv[1]) as fh:
    job = json.load(fh)
  out = {}
  for name in job["scenarios"]:
    _run_scenario(name, bool(job.get("graph")), out)
    print(f"variant_child: {name} done at {time.time() - t0:.2f} s", flush=True)
  np.savez(argv[2], **out)
  print(f"variant_child: ok, {len(out)} arrays, {time.time() - t0:.2f} s", flush=True)
  return 0


if __name__ == "__main__":
  sys.exit(main(sys.argv))
