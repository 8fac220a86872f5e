"""Observation history and delay in the fused HIP step (mjxObsState in include/mjx355_task.h,
csrc/obs_hist.h, mjlab_amd/fused.py FusedObsHistory) against the torch ObservationManager
(mjlab_amd/managers.py, mjlab_amd/buffers.py) on twin envs: same seed, same actions,
observation corruption off, timers out of reach, reset ranges zero (as tests/test_gpu_fused*.py).

Tolerances: those of the fused tests (fp32, operation order: rtol 1e-4, atol 1e-4); the
shift of a history block is a copy and is checked bit for bit.  The velocity command is
redrawn at a reset from different generators on the two paths, so its columns are compared
on the envs that did not reset only."""

import pytest
import torch

pytestmark = pytest.mark.gpu

G1, GO1 = "Mjlab-Velocity-Flat-Unitree-G1", "Mjlab-Velocity-Flat-Unitree-Go1"
JUMP, TRACK = "Mjlab-Jump-Flat-Unitree-G1", "Mjlab-Tracking-Flat-Unitree-G1"
N, STEPS, RESET_STEP = 64, 8, 3


def _env(task, n, device, fused, edit, capture=False, expect_fused=None):
  from mjlab_amd.envs import ManagerBasedRlEnv, load_env_cfg
  cfg = load_env_cfg(task, False)
  cfg.scene.num_envs = n
  cfg.seed = 3
  cfg.observations["policy"].enable_corruption = False
  if task == TRACK:
    for t in cfg.terminations.values():  # only time-outs end episodes
      if "threshold" in t.params:
        t.params["threshold"] = 1e6
    mc = cfg.commands["motion"]
    mc.pose_range, mc.velocity_range = {}, {}
    mc.joint_position_range = (0.0, 0.0)
    mc.sampling_mode = "start"
  else:
    cfg.events["reset_base"].params["pose_range"] = {}
    if task == JUMP:
      cfg.events["reset_robot_joints"].params["position_range"] = (0.0, 0.0)
  edit(cfg)
  env = ManagerBasedRlEnv(cfg, device=device)
  env.reset()
  env.enable_graph(capture=capture, fused=fused)
  if expect_fused is None:
    expect_fused = fused
  assert (env._fused is not None) == expect_fused, getattr(env, "_fused_unsupported", "")
  _quiet(env)
  return env


def _quiet(env):
  if "twist" in env.command_manager._terms:
    env.command_manager.get_term("twist").time_left.fill_(1e6)
  for tl in env.event_manager._interval_time_left:
    tl.fill_(1e6)


def _policy_history(h):
  def edit(cfg):
    cfg.observations["policy"].history_length = h
  return edit


def _mixed(cfg):
  for name in ("joint_pos", "joint_vel"):
    cfg.observations["policy"].terms[name].history_length = 3
  cfg.observations["critic"].history_length = 2


def _layout(env, group):
  """(term, width, history, first column) of a group's row, from the manager."""
  om = env.observation_manager
  out, off = [], 0
  for name, c, dim in zip(om._group_obs_term_names[group], om._group_obs_term_cfgs[group],
                          om._group_obs_term_dim[group]):
    h = max(int(c.history_length), 1)
    out.append((name, dim[0] // h, h, off))
    off += dim[0]
  assert (off,) == om.group_obs_dim[group]
  return out


def _comparable(env, group, task, was_reset):
  """[n, width] mask of the entries the two paths can agree on (see module docstring)."""
  n, width = env.num_envs, env.observation_manager.group_obs_dim[group][0]
  ok = torch.ones(n, width, dtype=torch.bool, device=env.device)
  if task in (G1, GO1):
    for name, w, h, off in _layout(env, group):
      if name == "command":
        ok[:, off:off + w * h] = ~was_reset[:, None]
  return ok


def _close(a, b):
  torch.testing.assert_close(a.float(), b.float(), rtol=1e-4, atol=1e-4)


def _run_twins(task, et, ef, device, steps=STEPS):
  """Steps the twins with the same actions; a third of the envs time out at RESET_STEP."""
  n = et.num_envs
  g = torch.Generator(device=device).manual_seed(0)
  nact = et.action_manager.total_action_dim
  was_reset = torch.zeros(n, dtype=torch.bool, device=device)
  prev = None
  for step in range(steps):
    if step == RESET_STEP:
      for e in (et, ef):
        e.episode_length_buf[::3] = e.max_episode_length - 1
    a = 0.3 * (2 * torch.rand(n, nact, device=device, generator=g) - 1)
    ot, _, tt, ut, _ = et.step(a)
    of, _, tf, uf, _ = ef.step(a)
    torch.cuda.synchronize()
    assert torch.equal(tt, tf) and torch.equal(ut, uf)
    done = tt | ut
    if step == RESET_STEP:
      assert done[::3].all()
    was_reset |= done
    of = {k: v.clone() for k, v in of.items()}
    for grp in ("policy", "critic"):
      assert of[grp].shape == ot[grp].shape == (n, et.observation_manager.group_obs_dim[grp][0])
      ok = _comparable(et, grp, task, was_reset)
      _close(torch.where(ok, ot[grp], 0), torch.where(ok, of[grp], 0))
      for name, w, h, off in _layout(ef, grp):
        blk = of[grp][:, off:off + w * h].reshape(n, h, w)
        if h > 1 and prev is not None:  # the shift is a copy
          old = prev[grp][:, off:off + w * h].reshape(n, h, w)
          assert torch.equal(blk[~done, :-1], old[~done, 1:]), (grp, name, step)
        if h > 1 and done.any():  # first append after the reset fills every slot
          assert torch.equal(blk[done], blk[done, -1:].expand(-1, h, -1)), (grp, name, step)
    prev = of
  assert was_reset.any() and not was_reset.all()


@pytest.mark.parametrize("task", [G1, GO1, JUMP, TRACK])
def test_policy_group_history_matches_torch(task, gpu_device):
  et = _env(task, N, gpu_device, False, _policy_history(3))
  ef = _env(task, N, gpu_device, True, _policy_history(3))
  frame = sum(w for _, w, _, _ in _layout(ef, "policy"))
  assert ef.observation_manager.group_obs_dim["policy"] == (3 * frame,)
  assert all(h == 1 for _, _, h, _ in _layout(ef, "critic"))
  _run_twins(task, et, ef, gpu_device)


@pytest.mark.parametrize("task", [G1, GO1])
def test_mixed_term_history_matches_torch(task, gpu_device):
  et = _env(task, N, gpu_device, False, _mixed)
  ef = _env(task, N, gpu_device, True, _mixed)
  hist = {name: h for name, _, h, _ in _layout(ef, "policy")}
  assert hist["joint_pos"] == hist["joint_vel"] == 3 and hist["actions"] == hist["command"] == 1
  assert all(h == 2 for _, _, h, _ in _layout(ef, "critic"))
  _run_twins(task, et, ef, gpu_device)


def test_hand_over_continues_the_history(gpu_device):
  """Torch steps, then the fused step is built: it must continue from the manager's buffers
  (not backfill), and hand them back when the env returns to the torch managers."""
  et = _env(G1, N, gpu_device, False, _policy_history(3))
  ef = _env(G1, N, gpu_device, False, _policy_history(3))
  g = torch.Generator(device=gpu_device).manual_seed(1)
  nact = et.action_manager.total_action_dim

  def both():
    a = 0.3 * (2 * torch.rand(N, nact, device=gpu_device, generator=g) - 1)
    ot, of = et.step(a)[0], ef.step(a)[0]
    torch.cuda.synchronize()
    for grp in ("policy", "critic"):
      _close(ot[grp], of[grp])
    return of["policy"]

  for _ in range(3):
    both()
  ef.enable_graph(capture=False, fused=True)
  assert ef._fused is not None, getattr(ef, "_fused_unsupported", "")
  _quiet(ef)
  pol = both()
  name, w, h, off = _layout(ef, "policy")[3]  # joint_pos: its three frames differ
  assert name == "joint_pos" and h == 3
  blk = pol[:, off:off + 3 * w].reshape(N, 3, w)
  assert not torch.equal(blk[:, 0], blk[:, 2])
  ef.enable_graph(capture=False, fused=False)  # releases the fused step
  assert ef._fused is None
  _quiet(ef)
  both()
  both()


def test_captured_fused_step_with_history(gpu_device):
  et = _env(G1, N, gpu_device, False, _policy_history(3))
  ef = _env(G1, N, gpu_device, True, _policy_history(3), capture=True)
  _run_twins(G1, et, ef, gpu_device)
  assert ef._graph is not None


def test_captured_torch_step_with_history(gpu_device):
  """The sync-free torch path (reset_masked, in-place buffers) records and replays."""
  et = _env(GO1, N, gpu_device, False, _mixed)
  ec = _env(GO1, N, gpu_device, False, _mixed, capture=True)
  _run_twins(GO1, et, ec, gpu_device)
  assert ec._graph is not None and ec._fused is None


def _delay(lo, hi, history=0, **policy):
  def edit(cfg):
    t = cfg.observations["policy"].terms["joint_pos"]
    t.delay_min_lag, t.delay_max_lag, t.history_length = lo, hi, history
    for k, v in policy.items():
      setattr(t, k, v)
  return edit


def test_constant_delay_matches_torch(gpu_device):
  et = _env(G1, N, gpu_device, False, _delay(2, 2, history=2))
  ef = _env(G1, N, gpu_device, True, _delay(2, 2, history=2))
  _run_twins(G1, et, ef, gpu_device, steps=7)  # the 3-frame ring wraps, across the reset
  assert (ef._fused._obs_hist.lags("policy", "joint_pos") == 2).all()


def test_random_delay_draws(gpu_device):
  n = 512
  ef = _env(GO1, n, gpu_device, True, _delay(0, 3))
  oh = ef._fused._obs_hist
  name, w, h, off = _layout(ef, "policy")[3]
  assert name == "joint_pos" and h == 1
  nact = ef.action_manager.total_action_dim
  g = torch.Generator(device=gpu_device).manual_seed(2)
  seen = set()
  for step in range(6):
    a = 0.3 * (2 * torch.rand(n, nact, device=gpu_device, generator=g) - 1)
    obs = ef.step(a)[0]["policy"]
    torch.cuda.synchronize()
    lags = oh.lags("policy", "joint_pos").long()
    pushes = oh.delay_pushes.long()
    assert int(lags.min()) >= 0 and int(lags.max()) <= 3
    assert (lags <= pushes - 1).all()
    seen |= set(lags.tolist())
    ring = oh.ring("policy", "joint_pos")  # [n, 4, w], oldest first
    want = ring[torch.arange(n, device=gpu_device), 3 - lags]
    assert torch.equal(obs[:, off:off + w], want)
    # the newest ring frame is this step's joint positions
    robot = ef.scene["robot"]
    _close(ring[:, 3], robot.data.joint_pos - robot.data.default_joint_pos)
  assert seen == {0, 1, 2, 3}


def test_other_delay_policies_fall_back_to_torch(gpu_device):
  env = _env(GO1, N, gpu_device, True, _delay(0, 3, delay_update_period=4), expect_fused=False)
  assert env._fused is None
  assert "delay policy" in env._fused_unsupported and "joint_pos" in env._fused_unsupported
  a = torch.zeros(N, env.action_manager.total_action_dim, device=gpu_device)
  for _ in range(2):
    obs = env.step(a)[0]
  torch.cuda.synchronize()
  assert torch.isfinite(obs["policy"]).all()
