"""The fused task kernels on constructed states against fp64 references.

test_gpu_fused*.py run the torch managers and the fused step side by side from a reset, where
a standing robot never falls, hardly lands a foot and tracks its motion with zero error.  Here
the tensors the descriptors point at are overwritten with seeded states that take every branch
(fused_inject.py: generators, coverage and tie rules, asserted without a GPU in
test_fused_states_cpu.py), one C-ABI entry point is called with no physics step in between,
and every output is compared with the fp64 numpy restatement of the same operation from the
same raw arrays:

  velocity (G1, Go1) and jump: mjx_task_post under both compiled forms of k_post
  (MJX355_TASK_POST_FORM 1 and 8, 40 envs = two full 16-wave blocks and a partial one), then
  the logs the following mjx_task_observe folds;
  tracking: mjx_track_post (k_post, k_log) at large tracking errors, then mjx_track_observe
  (k_cmd metrics, k_targets, k_obs) with no env at the motion end.

Tolerances, against fp64: flags, counts, episode lengths and termination logs exact; rewards
and episode sums rtol 1e-4, atol 1e-5; observations, targets and metrics atol 1e-4 (no rtol).
The Metrics/*_mean logs are means of fp32 sums: their bound is atol 1e-4 x max(1, largest
|summand|) -- the landing-force mean sums forces of up to 7,000 N (the excessive-force limit
is 2,500 N), one fp32 ulp of which is 4.9e-4.  Stateful values that are a max or one add of
values below 2 (peak heights, jump peak / initial, landing timer): atol 1e-6.
Every test prints its largest error / bound per output (DESIGN.md section 5 records them)."""

import os

import numpy as np
import pytest

import fused_inject as fi

pytestmark = pytest.mark.gpu

RW = dict(rtol=1e-4, atol=1e-5)
OBS = dict(rtol=0.0, atol=1e-4)
_envs, _outputs = {}, {}


def _task_env(family, form, device):
  """One env per (family, k_post form) and module; the form is read by mjx_task_create."""
  key = (family, form)
  if key not in _envs:
    old = os.environ.get("MJX355_TASK_POST_FORM")
    os.environ["MJX355_TASK_POST_FORM"] = str(form)
    try:
      _envs[key] = fi.build_env(family, device)
    finally:
      if old is None:
        del os.environ["MJX355_TASK_POST_FORM"]
      else:
        os.environ["MJX355_TASK_POST_FORM"] = old
  return _envs[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_envs():
  yield
  _envs.clear()
  _outputs.clear()


def _check(report, name, got, want, rtol, atol):
  r = fi.err_ratio(got, want, rtol, atol)
  report[name] = max(report.get(name, 0.0), r)
  assert r <= 1.0, f"{name}: largest error / bound = {r:.3g}"


def _exact(name, got, want):
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64)), \
      f"{name}: rows {np.nonzero(np.reshape(got.astype(np.int64) != want.astype(np.int64), (len(got), -1)).any(-1))[0]}"


def _desc_is_recorded(D, family):
  """The live descriptor is the recorded one the CPU generator checks ran on."""
  G = fi.golden_desc(family)
  diff = [k for k in G if k != "nworld" and G[k] != D.get(k)]
  assert not diff, f"tests/golden/fused_desc_{family}.json is stale in {diff}"


@pytest.mark.parametrize("form", [1, 8])
@pytest.mark.parametrize("family", ["g1", "go1", "jump"])
def test_task_post_on_constructed_states(family, form, gpu_device):
  env = _task_env(family, form, gpu_device)
  D = fi.live_desc(env)
  _desc_is_recorded(D, family)
  S, ref = fi.gen_task_state(D, seed=0)
  fi.assert_generator_ok(D, S, ref)
  tens = fi.task_tensors(env)
  fi.inject(tens, S)
  fi.call(env, "mjx_task_post")
  names = ["step_reward", "reward_buf", "episode_sums", "term_dones", "terminated", "time_outs",
           "reset_buf", "episode_length", "peak_heights"]
  jump = D["command_kind"] == fi.CMD_JUMP
  if jump:
    names += ["jump_peak", "jump_initial", "jump_initialized", "landing_timer", "was_in_air"]
  out = fi.fetch(tens, names)
  rep = {}
  for k in ("term_dones", "terminated", "time_outs", "reset_buf", "episode_length"):
    _exact(k, out[k], ref[k])
  kinds = D["reward_kind"][:D["nreward"]]
  for k, kind in enumerate(kinds):  # per term, so that the report names the term kind
    _check(rep, f"step_reward kind {kind}", out["step_reward"][:, k], ref["step_reward"][:, k], **RW)
    _check(rep, f"episode_sums kind {kind}", out["episode_sums"][:, k], ref["episode_sums"][:, k], **RW)
  _check(rep, "reward_buf", out["reward_buf"], ref["reward_buf"], **RW)
  _check(rep, "peak_heights", out["peak_heights"], ref["peak_heights"], rtol=0.0, atol=1e-6)
  if jump:
    _exact("jump_initialized", out["jump_initialized"], ref["jump_initialized"])
    _exact("was_in_air", out["was_in_air"], ref["was_in_air"])
    for k in ("jump_peak", "jump_initial", "landing_timer"):
      _check(rep, k, out[k], ref[k], rtol=0.0, atol=1e-6)
  # all-NaN cvel row: every term that reads it gives zero; NaN root orientation: no termination
  assert np.isfinite(out["step_reward"]).all() and np.isfinite(out["reward_buf"]).all()
  # ---- the logs of this step's resets, folded by the next observe
  fi.call(env, "mjx_task_observe")
  fz = env._fused
  log = {k: v.detach().cpu().numpy() for k, v in
         (("reward", fz.log_reward), ("term", fz.log_term), ("cmd", fz.log_cmd), ("metric", fz.log_metric))}
  _exact("Episode_Termination", log["term"][:D["ntermination"]], ref["log_termination"])
  _check(rep, "Episode_Reward", log["reward"][:D["nreward"]], ref["log_reward"], **RW)
  _check(rep, "Metrics/command errors", log["cmd"], ref["log_command"], **OBS)
  fmax = float(np.abs(S["sensordata"]).max())
  for m, key in enumerate(("angular_momentum", "air_time", "peak_height", "slip_velocity", "landing_force",
                           "peak_jump_height", "jump_height", "landing_success_rate")):
    scale = max(1.0, fmax) if key == "landing_force" else 1.0
    _check(rep, f"Metrics/{key}", log["metric"][m], ref["log_metric"][m], rtol=0.0, atol=1e-4 * scale)
  # the two forms' per-env outputs: recorded, not required to be bit-identical
  _outputs[(family, form)] = out
  other = _outputs.get((family, 9 - form))
  if other is not None:
    same = all(np.array_equal(out[k], other[k], equal_nan=True) for k in names)
    print(f"\n[{family}] k_post<1> and k_post<8> per-env outputs bit-identical: {same}")
  print(f"\n[{family} k_post<{form}>] largest error / bound:",
        ", ".join(f"{k} {v:.2g}" for k, v in sorted(rep.items())))


def test_task_post_edge_rows(gpu_device):
  """The deterministic rows, read back explicitly (Go1 carries every feet term at a weight):
  four fp32 accumulations of 0.005f are a first contact, five and zero are not; an air time
  exactly on threshold_min / threshold_max earns nothing; joints exactly on a soft limit
  cost nothing; episode_length + 1 == max_episode_length times out."""
  env = _task_env("go1", 1, gpu_device)
  D = fi.live_desc(env)
  S, ref = fi.gen_task_state(D, seed=0)
  tens = fi.task_tensors(env)
  fi.inject(tens, S)
  fi.call(env, "mjx_task_post")
  out = fi.fetch(tens, ["step_reward", "peak_heights", "time_outs", "terminated", "term_dones"])
  kinds = D["reward_kind"][:D["nreward"]]
  col = {kind: k for k, kind in enumerate(kinds)}
  sw, sl, at, lim = (col[k] for k in (fi.RW_FEET_SWING, fi.RW_SOFT_LANDING, fi.RW_FEET_AIR_TIME,
                                       fi.RW_JOINT_POS_LIMITS))
  assert out["step_reward"][0, sl] < 0 and (out["peak_heights"][0] == 0).all()       # landed: peaks reset
  assert out["step_reward"][0, sw] < 0
  for row in (1, 2):
    assert out["step_reward"][row, sl] == 0 and out["step_reward"][row, sw] == 0
    assert (out["peak_heights"][row] > 0).all()
  assert out["step_reward"][3, at] == 0
  assert out["step_reward"][4, lim] == 0
  assert out["time_outs"][5] and not out["terminated"][5]
  assert not out["term_dones"][1, 7]  # NaN orientation: bad_orientation stays false
  fi.call(env, "mjx_task_observe")    # fold the partials before the env is used again


def test_track_post_and_observe_at_large_errors(gpu_device):
  env = fi.build_env("tracking", gpu_device)
  D = fi.live_desc(env)
  D["motion_T"] = D["nframe"]
  _desc_is_recorded(D, "tracking")
  M = fi.motion_arrays(env)
  origins = env.scene.env_origins.cpu().numpy()
  bias = env._fused._cmd.robot.data.encoder_bias.cpu().numpy()
  S, ref = fi.gen_track_state(D, M, origins, seed=0)
  fi.assert_track_generator_ok(D, ref)
  tens = fi.track_tensors(env)
  fi.inject(tens, S)
  fi.call(env, "mjx_track_post")
  out = fi.fetch(tens, ["step_reward", "reward_buf", "episode_sums", "term_dones", "terminated",
                        "time_outs", "reset_buf", "episode_length"])
  rep = {}
  for k in ("term_dones", "terminated", "time_outs", "reset_buf", "episode_length"):
    _exact(k, out[k], ref[k])
  for k in range(D["nreward"]):
    kind = D["reward_kind"][k]
    _check(rep, f"step_reward kind {kind}", out["step_reward"][:, k], ref["step_reward"][:, k], **RW)
    _check(rep, f"episode_sums kind {kind}", out["episode_sums"][:, k], ref["episode_sums"][:, k], **RW)
  _check(rep, "reward_buf", out["reward_buf"], ref["reward_buf"], **RW)
  fz = env._fused
  _exact("Episode_Termination", fz.log_term.cpu().numpy()[:D["ntermination"]], ref["log_termination"])
  _check(rep, "Episode_Reward", fz.log_reward.cpu().numpy()[:D["nreward"]], ref["log_reward"], **RW)
  _check(rep, "Metrics/motion log", fz.log_metric.cpu().numpy(), ref["log_metric"], **OBS)
  # ---- observe on the same state: metrics on the injected targets, then targets and
  # observations at the next frame (the injected post state is kept: no reset ran)
  want = fi.ref_track_observe(D, M, origins, bias, S)
  fi.call(env, "mjx_track_observe")
  got = fi.fetch(tens, ["metrics", "time_steps", "body_pos_rel", "body_quat_rel", "resample_mask"])
  _exact("time_steps", got["time_steps"], want["time_steps"])
  assert not got["resample_mask"].any()
  for m, name in enumerate(fi_metric_names()):
    _check(rep, f"metric {name}", got["metrics"][:, m], want["metrics"][:, m], **OBS)
  _check(rep, "body_pos_relative_w", got["body_pos_rel"], want["body_pos_rel"], **OBS)
  _check(rep, "body_quat_relative_w", got["body_quat_rel"], want["body_quat_rel"], **OBS)
  _check(rep, "obs critic", fz.obs["critic"].cpu().numpy(), want["critic"], **OBS)
  _check(rep, "obs policy", fz.obs["policy"].cpu().numpy(), want["policy"], **OBS)
  print("\n[tracking] largest error / bound:", ", ".join(f"{k} {v:.2g}" for k, v in sorted(rep.items())))


def fi_metric_names():
  from mjlab_amd.fused_tracking import METRIC_NAMES
  return METRIC_NAMES[:10]
