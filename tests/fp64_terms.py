"""fp64 numpy restatements of the reference formulas, shared by the CPU term tests
(test_host_logic.py, test_tracking_terms.py) and the fused-kernel tests on constructed
states (fused_inject.py, test_gpu_fused_states.py, test_gpu_fused_sampling.py).

Every function takes numpy arrays (any float dtype, promoted to float64), broadcasts over
leading axes and cites the reference text it restates.  Quaternions are (w, x, y, z)."""

import numpy as np

F = np.float64


def f64(a):
  return np.asarray(a, dtype=F)


# ------------------------------------------------------------------ utils/lab_api/math.py
def quat_mul(a, b):
  a, b = f64(a), f64(b)
  w1, x1, y1, z1 = (a[..., i] for i in range(4))
  w2, x2, y2, z2 = (b[..., i] for i in range(4))
  return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                   w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def quat_conj(q):
  return f64(q) * np.array([1.0, -1.0, -1.0, -1.0])


def quat_inv(q):
  """math.py quat_inv: conjugate over the squared norm."""
  q = f64(q)
  return quat_conj(q) / np.sum(q * q, -1, keepdims=True)


def quat_apply(q, v):
  """math.py:629-650: v + w t + u x t, t = 2 u x v."""
  q, v = f64(q), f64(v)
  u = q[..., 1:]
  t = 2.0 * np.cross(u, v)
  return v + q[..., :1] * t + np.cross(u, t)


def quat_apply_inverse(q, v):
  """math.py:653-670."""
  q, v = f64(q), f64(v)
  u = q[..., 1:]
  t = 2.0 * np.cross(u, v)
  return v - q[..., :1] * t + np.cross(u, t)


def quat_error_magnitude(a, b):
  """math.py:478-506, 688-699: |axis_angle(a * conj(b))|."""
  q = quat_mul(a, quat_conj(b))
  q = q * np.where(q[..., :1] < 0.0, -1.0, 1.0)
  mag = np.linalg.norm(q[..., 1:], axis=-1)
  half = np.arctan2(mag, q[..., 0])
  ang = 2.0 * half
  with np.errstate(divide="ignore", invalid="ignore"):
    s = np.where(np.abs(ang) > 1e-6, np.sin(half) / ang, 0.5 - ang * ang / 48.0)
  return mag / np.abs(s)


def yaw_quat(q):
  """math.py:566-588."""
  q = f64(q)
  w, x, y, z = (q[..., i] for i in range(4))
  yaw = np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))
  o = np.zeros_like(q)
  o[..., 0], o[..., 3] = np.cos(0.5 * yaw), np.sin(0.5 * yaw)
  return o


def matrix_from_quat(q):
  """math.py:166-196, [..., 3, 3]."""
  q = f64(q)
  w, x, y, z = (q[..., i] for i in range(4))
  m = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)
  return m.reshape(q.shape[:-1] + (3, 3))


def rot6d(q):
  """observations.py:33-45: the first two columns of the rotation matrix, row-major."""
  return matrix_from_quat(q)[..., :2].reshape(np.shape(q)[:-1] + (6,))


# ------------------------------------------------------------------ entity/data.py
def link_lin_vel(cvel, com, pos):
  """entity/data.py body_link_lin_vel_w / site_lin_vel_w: cvel = (angular, linear at the
  root's subtree com); the linear velocity at `pos` is lin - ang x (com - pos)."""
  cvel = f64(cvel)
  return cvel[..., 3:6] - np.cross(cvel[..., 0:3], f64(com) - f64(pos))


def projected_gravity(q):
  return quat_apply_inverse(q, np.array([0.0, 0.0, -1.0]))


# ------------------------------------------------------------------ tasks/velocity/mdp/rewards.py
def command_speed(c):
  c = f64(c)
  return np.linalg.norm(c[..., :2], axis=-1) + np.abs(c[..., 2])


def command_active(c, thr):
  """The command gate of the feet terms (rewards.py:147-151)."""
  return (command_speed(c) > thr).astype(F)


def track_linear_velocity(c, v, std):
  """rewards.py:23-40."""
  c, v = f64(c), f64(v)
  return np.exp(-(np.sum((c[..., :2] - v[..., :2]) ** 2, -1) + v[..., 2] ** 2) / std ** 2)


def track_angular_velocity(c, w, std):
  """rewards.py:43-60."""
  c, w = f64(c), f64(w)
  return np.exp(-((c[..., 2] - w[..., 2]) ** 2 + np.sum(w[..., :2] ** 2, -1)) / std ** 2)


def flat_orientation(g, std):
  """rewards.py:63-85 on the projected gravity of the root or of the named body."""
  return np.exp(-np.sum(f64(g)[..., :2] ** 2, -1) / std ** 2)


def variable_posture(q, default, std_standing, std_walking, std_running, c, p0, p1):
  """rewards.py:291-359: std table by command speed, exp(-mean(err^2 / std^2))."""
  speed = command_speed(c)[..., None]
  std = np.where(speed < p0, f64(std_standing), np.where(speed < p1, f64(std_walking), f64(std_running)))
  return np.exp(-np.mean((f64(q) - f64(default)) ** 2 / std ** 2, -1))


def joint_pos_limits(q, lo, hi):
  """envs/mdp/rewards.py:73-88."""
  q = f64(q)
  return np.sum(-np.minimum(q - f64(lo), 0.0) + np.maximum(q - f64(hi), 0.0), -1)


def action_rate_l2(a, pa):
  """envs/mdp/rewards.py:56-60."""
  return np.sum((f64(a) - f64(pa)) ** 2, -1)


def action_acc_l2(a, pa, ppa):
  """envs/mdp/rewards.py:63-70."""
  return np.sum((f64(a) - 2.0 * f64(pa) + f64(ppa)) ** 2, -1)


def first_contact(cc, dt, abs_tol=1e-8):
  """sensor/contact_sensor.py:260-270, on fp32 contact times: the window's upper edge is the
  fp32 sum dt + abs_tol, as the reference's float32 tensors compare."""
  cc = np.asarray(cc, dtype=np.float32)
  return (cc > 0) & (cc < np.float32(np.float32(dt) + np.float32(abs_tol)))


def feet_air_time(air, p0, p1, c, thr):
  """rewards.py:123-152."""
  air = f64(air)
  return np.sum((air > p0) & (air < p1), -1) * command_active(c, thr)


def feet_clearance(z, vxy, target, c, thr):
  """rewards.py:155-177; vxy is the [.., 2] horizontal site velocity."""
  return np.sum(np.abs(f64(z) - target) * np.linalg.norm(f64(vxy), axis=-1), -1) * command_active(c, thr)


def feet_slip(vxy, found, c, thr):
  """rewards.py:232-259."""
  return np.sum(np.sum(f64(vxy) ** 2, -1) * (f64(found) > 0), -1) * command_active(c, thr)


def soft_landing(force, first, gate):
  """rewards.py:262-288; gate = command_active(...) or 1 with no command."""
  return np.sum(np.linalg.norm(f64(force), axis=-1) * first, -1) * gate


def swing_height(peak, z, found, first, target, gate):
  """rewards.py:180-229: returns (cost, peak heights after the step)."""
  peak = np.where(f64(found) == 0, np.maximum(f64(peak), f64(z)), f64(peak))
  cost = np.sum((peak / target - 1.0) ** 2 * first, -1) * gate
  return cost, np.where(first, 0.0, peak), peak


# ------------------------------------------------------------------ tasks/tracking/mdp
def exp_kernel(err2, std):
  """rewards.py:26-120: exp(-err / std^2)."""
  return np.exp(-f64(err2) / std ** 2)


def relative_targets(anchor_pos, anchor_quat, robot_anchor_pos, robot_anchor_quat, body_pos,
                     body_quat):
  """commands.py:383-405: motion bodies yaw-aligned to the robot anchor; anchors [N, 3|4],
  bodies [N, nb, 3|4].  Returns (body_pos_relative_w, body_quat_relative_w)."""
  ap, rp = f64(anchor_pos)[:, None, :], f64(robot_anchor_pos)[:, None, :]
  delta_pos = np.concatenate([np.broadcast_to(rp[..., :2], ap[..., :2].shape), ap[..., 2:3]], -1)
  delta_ori = yaw_quat(quat_mul(robot_anchor_quat, quat_inv(anchor_quat)))[:, None, :]
  return delta_pos + quat_apply(delta_ori, f64(body_pos) - ap), quat_mul(delta_ori, body_quat)


def sampling_probabilities(bin_failed_count, uniform_ratio, kernel):
  """commands.py:272-290: uniform floor, non-causal kernel with replicate padding on the
  right, normalised."""
  b = f64(bin_failed_count)
  n, k = b.shape[0], f64(kernel)
  base = b + uniform_ratio / float(n)
  padded = np.concatenate([base, np.repeat(base[-1:], len(k) - 1)])
  p = np.array([np.dot(padded[i:i + len(k)], k) for i in range(n)])
  return p / p.sum()


def sampling_metrics(p):
  """commands.py:293-300: (normalised entropy, top-1 probability, top-1 bin / bin count)."""
  p = f64(p)
  n = p.shape[0]
  h = -np.sum(p * np.log(p + 1e-12))
  return np.array([h / np.log(n), p.max(), float(np.argmax(p)) / n])


def current_bins(time_steps, bin_count, nframe):
  """commands.py:261-266."""
  ts = np.asarray(time_steps, dtype=np.int64)
  return np.clip((ts * bin_count) // max(int(nframe), 1), 0, bin_count - 1)
