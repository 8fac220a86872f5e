"""Cost of the extended sensors (csrc/sensor_ext.hip): G1 velocity flat, 4,096 envs, the fused
captured env step with and without eight extended sensors added through cfg.scene.sensors, as
env-steps/s over alternating windows (without, with, without, with, ...), each window in a child
process of its own under its own time limit; the parent never opens the GPU.  The scene with the
sensors matches no compiled specs.inc entry and runs kernels specialised at run time
(mjlab_amd.jit): --prebuild compiles them into the in-tree cache (no GPU needed) so that no
window pays the compile.  Prints one JSON line.
usage: bench_sensor_kinds.py [--num-envs 4096] [--steps 100] [--warmup 20] [--windows 3] [--limit 240]
       bench_sensor_kinds.py --prebuild"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mjlab-1_amd"))
TASK = "Mjlab-Velocity-Flat-Unitree-G1"


def make_cfg(num_envs, sensors):
  from mjlab_amd.envs import load_env_cfg
  from mjlab_amd.sensor import BuiltinSensorCfg, ObjRef
  cfg = load_env_cfg(TASK, False)
  cfg.scene.num_envs = num_envs
  if sensors:
    o = lambda t, n: ObjRef(t, n, entity="robot")
    cfg.scene.sensors = cfg.scene.sensors + (
      BuiltinSensorCfg("x_com", "subtreecom", o("body", "pelvis")),
      BuiltinSensorCfg("x_com_vel", "subtreelinvel", o("body", "pelvis")),
      BuiltinSensorCfg("x_lfoot", "framepos", o("site", "left_foot"), ref=o("xbody", "pelvis")),
      BuiltinSensorCfg("x_rfoot", "framepos", o("site", "right_foot"), ref=o("xbody", "pelvis")),
      BuiltinSensorCfg("x_torso_quat", "framequat", o("xbody", "torso_link"), ref=o("xbody", "pelvis")),
      BuiltinSensorCfg("x_foot_vel", "framelinvel", o("site", "right_foot"), ref=o("site", "imu_in_pelvis")),
      BuiltinSensorCfg("x_palm_acc", "framelinacc", o("site", "left_palm"), cutoff=50.0),
      BuiltinSensorCfg("x_knee_frc", "jointactuatorfrc", o("joint", "left_knee_joint")))
  return cfg


def prebuild(num_envs):
  from mjlab_amd import jit
  from mjlab_amd.scene import Scene
  from mjlab_amd.sim.sim import max_capacity, world_capacity
  cfg = make_cfg(num_envs, True)
  model = Scene(cfg.scene, "cpu").compile()
  cfg.sim.mujoco.apply(model)
  fast, big = world_capacity(cfg.sim, model), max_capacity(cfg.sim, model)
  jit.prebuild([(model, fast[0], fast[1], 1)] + ([(model, big[0], big[1], 2)] if big != fast else []))


def child(sensors, num_envs, steps, warmup):
  import ctypes
  import torch
  from mjlab_amd._lib import check, lib
  from mjlab_amd.envs import ManagerBasedRlEnv
  env = ManagerBasedRlEnv(make_cfg(num_envs, sensors), device="cuda:0")
  env.reset()
  env.enable_graph(capture=True, fused=True)
  assert env._fused is not None, env._fused_unsupported
  act = torch.zeros(num_envs, env.action_manager.total_action_dim, device="cuda:0")
  for _ in range(warmup):
    env.step(act)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(steps):
    env.step(act)
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  n = (ctypes.c_int64 * 1)()
  check(lib().mjx_sensor_launch_count(n))
  print(json.dumps({"sensors": 8 if sensors else 0, "env_steps_per_s": num_envs * steps / dt,
                    "ms_per_env_step": 1e3 * dt / steps, "spec": env.sim.info()["spec"],
                    "sensor_launches_recorded": int(n[0])}))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--num-envs", type=int, default=4096)
  ap.add_argument("--steps", type=int, default=100)
  ap.add_argument("--warmup", type=int, default=20)
  ap.add_argument("--windows", type=int, default=3)
  ap.add_argument("--limit", type=int, default=240, help="seconds per window")
  ap.add_argument("--prebuild", action="store_true")
  ap.add_argument("--child", default=None)
  a = ap.parse_args()
  if a.prebuild:
    prebuild(a.num_envs)
    return
  if a.child:
    child(a.child == "with", a.num_envs, a.steps, a.warmup)
    return
  out = {"task": TASK, "num_envs": a.num_envs, "steps": a.steps, "windows": []}
  for _ in range(a.windows):
    for mode in ("without", "with"):
      cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", mode,
             "--num-envs", str(a.num_envs), "--steps", str(a.steps), "--warmup", str(a.warmup)]
      r = subprocess.run(cmd, capture_output=True, text=True)
      if r.returncode != 0:  # nothing more is started on the GPU after a failure
        print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
        raise SystemExit(f"bench_sensor_kinds: window {mode} ended with status {r.returncode}")
      out["windows"].append(json.loads(r.stdout.strip().splitlines()[-1]))
  for mode, k in (("without", 0), ("with", 8)):
    v = [w["env_steps_per_s"] for w in out["windows"] if w["sensors"] == k]
    out[mode] = {"env_steps_per_s_mean": sum(v) / len(v), "min": min(v), "max": max(v)}
  out["cost_percent"] = 100.0 * (1.0 - out["with"]["env_steps_per_s_mean"] / out["without"]["env_steps_per_s_mean"])
  print(json.dumps(out))


if __name__ == "__main__":
  main()
