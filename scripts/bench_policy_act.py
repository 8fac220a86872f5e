"""Cost of the rollout-time policy evaluation `PPO.act` at the G1 velocity shapes (4,096 envs,
actor 99-512-256-128-29, critic 111-512-256-128-1, elu, both normalisers on), as microseconds
per call of
  graph   PPO.act on the graph path (graph_act: ~40 torch kernels replayed as one graph)
  fused   PPO.act with fused_act=True (one launch of csrc/policy.hip into the storage rows)
Both variants share one policy and run alternately in one process, `--rounds` windows each of
`--calls` calls after `--warmup`, timed with device events around the window and a synchronise
at its end.  Prints one line per window, then one JSON line with each variant's median and
run-to-run spread (max - min over its windows).
usage: bench_policy_act.py [--num-envs 4096] [--calls 200] [--warmup 50] [--rounds 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mjlab-1_amd"))
NA_OBS, NC_OBS, HIDDEN, NACT, T = 99, 111, (512, 256, 128), 29, 24


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--num-envs", type=int, default=4096)
  ap.add_argument("--calls", type=int, default=200)
  ap.add_argument("--warmup", type=int, default=50)
  ap.add_argument("--rounds", type=int, default=3)
  ap.add_argument("--only", choices=("graph", "fused"), default=None, help="one variant (kernel traces)")
  a = ap.parse_args()
  import torch
  from mjlab_amd.rl.ppo import PPO, ActorCritic
  dev, n = "cuda:0", a.num_envs
  torch.manual_seed(0)
  obs = {"policy": torch.randn(n, NA_OBS, device=dev), "critic": torch.randn(n, NC_OBS, device=dev)}
  policy = ActorCritic(obs, {"policy": ["policy"], "critic": ["critic"]}, NACT, actor_obs_normalization=True,
                       critic_obs_normalization=True, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN)
  algs = {"graph": PPO(policy, device=dev), "fused": PPO(policy, device=dev, fused_act=True)}
  if a.only:
    algs = {a.only: algs[a.only]}
  for alg in algs.values():
    alg.init_storage(n, T, obs, NACT)

  def window(alg, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(calls):
      alg.storage.step = i % T
      alg.act(obs)
    end.record()
    torch.cuda.synchronize()
    return 1e3 * start.elapsed_time(end) / calls

  us = {k: [] for k in algs}
  with torch.inference_mode():
    for alg in algs.values():
      window(alg, a.warmup)
    for r in range(a.rounds):
      for k, alg in algs.items():
        us[k].append(window(alg, a.calls))
        print(f"round {r} {k:5s} {us[k][-1]:8.1f} us per PPO.act")
  out = {"num_envs": n, "calls": a.calls, "rounds": a.rounds}
  for k, v in us.items():
    out[k] = {"median_us": statistics.median(v), "spread_us": max(v) - min(v), "windows_us": v}
  if "fused" in algs:
    out["fused_launches"] = algs["fused"]._fused.launches
  print(json.dumps(out))


if __name__ == "__main__":
  main()
