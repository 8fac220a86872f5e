"""The CPU half of the constructed-state tests of the fused kernels (test_gpu_fused_states.py,
test_gpu_fused_sampling.py): the shared fp64 formulas against closed forms, and the state
generators of fused_inject.py against their contract, asserted on the fp64 reference alone:
no random row within 1e-5 * max(1, |threshold|) of a comparison threshold, every listed
branch taken by at least 4 rows, and for the tracking task at least half of the rows of every
exp-kernel reward in [0.05, 0.95].  The descriptors are the recorded ones of the test envs
(tests/golden/fused_desc_*.json; the GPU tests assert that the live descriptors equal them)."""

import numpy as np
import pytest

import fp64_terms as T
import fused_inject as fi


# ------------------------------------------------------------------ formulas
def test_quat_formulas_against_closed_forms():
  rng = np.random.default_rng(0)
  q = rng.standard_normal((64, 4))
  q /= np.linalg.norm(q, axis=-1, keepdims=True)
  v = rng.standard_normal((64, 3))
  R = T.matrix_from_quat(q)
  np.testing.assert_allclose(T.quat_apply(q, v), np.einsum("nij,nj->ni", R, v), atol=1e-14)
  np.testing.assert_allclose(T.quat_apply_inverse(q, T.quat_apply(q, v)), v, atol=1e-14)
  np.testing.assert_allclose(T.quat_mul(q, T.quat_inv(q)), np.tile([1.0, 0, 0, 0], (64, 1)), atol=1e-14)
  ang = np.array([0.0, 1e-7, 0.3, 1.0, 3.0])
  qz = np.stack([np.cos(ang / 2), 0 * ang, 0 * ang, np.sin(ang / 2)], -1)
  np.testing.assert_allclose(T.quat_error_magnitude(qz, np.array([1.0, 0, 0, 0])), ang, atol=1e-12)
  np.testing.assert_allclose(T.quat_error_magnitude(-qz, qz), 0.0, atol=1e-12)
  np.testing.assert_allclose(T.yaw_quat(qz), qz, atol=1e-14)
  np.testing.assert_allclose(T.projected_gravity(np.array([1.0, 0, 0, 0])), [0, 0, -1])
  # a rigid body turning about z through the com: the point at +x moves along +y
  cvel = np.array([0, 0, 2.0, 0, 0, 0])
  np.testing.assert_allclose(T.link_lin_vel(cvel, np.zeros(3), np.array([1.0, 0, 0])), [0, 2.0, 0])


def test_relative_targets_identity_and_yaw():
  rng = np.random.default_rng(1)
  n, nb = 5, 4
  bp = rng.standard_normal((n, nb, 3))
  bq = rng.standard_normal((n, nb, 4))
  bq /= np.linalg.norm(bq, axis=-1, keepdims=True)
  p, q = T.relative_targets(bp[:, 1], bq[:, 1], bp[:, 1], bq[:, 1], bp, bq)
  np.testing.assert_allclose(p, bp, atol=1e-12)
  np.testing.assert_allclose(T.quat_error_magnitude(q, bq), 0.0, atol=1e-7)
  psi = 0.7
  qy = np.array([np.cos(psi / 2), 0, 0, np.sin(psi / 2)])
  p, q = T.relative_targets(bp[:, 1], bq[:, 1], bp[:, 1] + [0.5, -0.2, 0.9], T.quat_mul(qy, bq[:, 1]), bp, bq)
  want = T.quat_apply(qy, bp - bp[:, 1:2]) + bp[:, 1:2] + [0.5, -0.2, 0.0]  # z stays the motion's
  np.testing.assert_allclose(p, want, atol=1e-12)
  np.testing.assert_allclose(T.quat_error_magnitude(q, T.quat_mul(qy, bq)), 0.0, atol=1e-7)


def test_first_contact_window_in_fp32():
  """sensor/contact_sensor.py:260-270 on fp32 timers: four accumulations of 0.005f are
  exactly 0.02f and inside the window, five are not, zero is not; the window's upper edge
  float32(0.02 + 1e-8) is excluded."""
  f32 = np.float32
  acc = [f32(0)]
  for _ in range(5):
    acc.append(f32(acc[-1] + f32(0.005)))
  assert acc[4] == f32(0.02)
  cc = np.array([acc[4], acc[5], 0.0, np.nextafter(f32(0.02), f32(1)), f32(0.02 + 1e-8)], dtype=f32)
  assert T.first_contact(cc, 0.02).tolist() == [True, False, False, True, False]


def test_sampling_formulas():
  k = np.array([0.8 ** i for i in range(3)])
  k /= k.sum()
  b = np.zeros(11)
  b[4] = 1.0
  p = T.sampling_probabilities(b, 0.1, k)
  assert abs(p.sum() - 1.0) < 1e-15 and int(np.argmax(p)) == 4
  np.testing.assert_allclose(p[5:], p[5])                    # replicate padding: a flat tail
  base = b + 0.1 / 11
  np.testing.assert_allclose(p[2] * (k @ base[4:7]), p[4] * (k @ base[2:5]))
  h, pmax, top = T.sampling_metrics(np.full(8, 0.125))
  assert abs(h - 1.0) < 1e-9 and pmax == 0.125 and top == 0.0
  assert T.current_bins([0, 249, 250, 499, 500], 11, 500).tolist() == [0, 5, 5, 10, 10]


# ------------------------------------------------------------------ generators
@pytest.mark.parametrize("family", ["g1", "go1", "jump"])
def test_task_state_generator(family):
  D = fi.golden_desc(family)
  S, ref = fi.gen_task_state(D, seed=0)
  assert S["qpos"].shape[0] == fi.N_ENVS
  fi.assert_generator_ok(D, S, ref)
  kinds = D["termination_kind"][:D["ntermination"]]
  ori = kinds.index(fi.TM_BAD_ORIENT)
  assert 0.3 <= ref["term_dones"][ori].mean() <= 0.6      # roughly half of the rows fall over
  used = set(D["reward_kind"][:D["nreward"]])
  assert fi.RW_IS_ALIVE not in used or ref["terminated"].any()
  # deterministic rows: 0 lands every foot, 1 and 2 none; 4 sits on the soft limits; 5 times out;
  # 6 (NaN cvel) and 7 (NaN root orientation) give finite rewards and no orientation termination
  assert np.isfinite(ref["step_reward"]).all() and np.isfinite(ref["reward_buf"]).all()
  assert ref["time_outs"][5] and not ref["terminated"][5]
  assert not ref["term_dones"][ori, 7] and not ref["term_dones"][ori, 6]
  col = {kind: k for k, kind in enumerate(D["reward_kind"][:D["nreward"]])}
  assert ref["step_reward"][4, col[fi.RW_JOINT_POS_LIMITS]] == 0
  sl = col[fi.RW_SOFT_LANDING]
  assert ref["step_reward"][0, sl] < 0 and ref["step_reward"][1, sl] == 0 and ref["step_reward"][2, sl] == 0
  if fi.RW_TRACK_LIN in col:
    assert ref["step_reward"][6, col[fi.RW_TRACK_LIN]] == 0  # reads the NaN cvel: nan_to_num


def test_every_shipped_term_kind_runs_at_a_weight():
  """Every reward and termination kind of the shipped velocity / jump configs is evaluated at
  a non-zero weight by one of the three test envs, and one env keeps a zero-weight term."""
  seen, zero = set(), False
  for family in ("g1", "go1", "jump"):
    D = fi.golden_desc(family)
    for k in range(D["nreward"]):
      if D["reward_weight"][k] != 0.0:
        seen.add(D["reward_kind"][k])
      else:
        zero = True
  assert seen == set(range(24)) and zero
  terms = {k for f in ("g1", "go1", "jump") for k in fi.golden_desc(f)["termination_kind"][:fi.golden_desc(f)["ntermination"]]}
  assert terms == set(range(5))


@pytest.mark.parametrize("seed", [0, 1])
def test_track_state_generator(seed):
  D = fi.golden_desc("tracking")
  M = fi.standin_motion(D)
  origins = np.random.default_rng(5).standard_normal((fi.N_ENVS, 3)) * [3.0, 3.0, 0.0]
  S, ref = fi.gen_track_state(D, M, origins.astype(np.float32), seed=seed)
  fi.assert_track_generator_ok(D, ref)
  assert set(D["termination_kind"][:D["ntermination"]]) == set(range(6))
  assert set(D["reward_kind"][:D["nreward"]]) == set(range(9))
  assert S["time_steps"].min() == 0 and S["time_steps"].max() == D["nframe"] - 2  # the whole motion
  obs = fi.ref_track_observe(D, M, origins, np.zeros((fi.N_ENVS, D["njoint"])), S)
  assert obs["critic"].shape == (fi.N_ENVS, D["ncritic"]) and obs["policy"].shape == (fi.N_ENVS, D["npolicy"])
