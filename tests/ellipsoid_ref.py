"""Independent fp64 geometry of the ellipsoid narrowphase tests (numpy only; no engine, no oracle).
An ellipsoid is narrowphase_ref's Shape of kind ELLIPSOID, size = its semi-axes.  Its nearest point
comes from the secular equation sum (s_i p_i / (t + s_i^2))^2 = 1, bisected in u = t + s_min^2 to
1e-14.  `support` is the ellipsoid's; cylinder_ref's `project`, `height` and `signed_distance` are wrapped (kind 4,
and the capsule's height) and put back, so its `closest` and depth functions apply to ellipsoid pairs unchanged."""

import math

import numpy as np

import cylinder_ref as C
from narrowphase_ref import CAPSULE

ELLIPSOID = 4


def nearest(p, s, surface=False):
  """The point of the solid (surface=True: of the surface, also for p inside) nearest p, shape frame."""
  p, s = [float(v) for v in p], [float(v) for v in s]
  q = sum((p[i] / s[i]) ** 2 for i in range(3))
  if q <= 1.0 and not surface:
    return np.array(p)
  m = min(range(3), key=lambda i: s[i])
  e = [s[i] ** 2 - s[m] ** 2 for i in range(3)]
  y = [s[i] * abs(p[i]) for i in range(3)]
  lo, hi = (s[m] ** 2, max(math.hypot(*y), s[m] ** 2)) if q > 1.0 else (0.0, s[m] ** 2)
  while hi - lo > 1e-14 * hi and hi > 1e-300:  # F decreases: positive left of the root
    u = 0.5 * (lo + hi)
    if sum((y[i] / (u + e[i])) ** 2 for i in range(3)) > 1.0:
      lo = u
    else:
      hi = u
  x = [s[i] ** 2 * p[i] / (hi + e[i]) if i != m and hi + e[i] > 0 else 0.0 for i in range(3)]
  # (the smallest axis' coordinate from the surface equation: also right on its symmetry plane)
  x[m] = math.copysign(s[m] * math.sqrt(max(1.0 - sum((x[i] / s[i]) ** 2 for i in range(3) if i != m), 0.0)), p[m])
  return np.array(x)


_signed_distance, _project, _height = C.signed_distance, C.project, C.height


def signed_distance(S, pw):
  if S.kind != ELLIPSOID:
    return _signed_distance(S, pw)
  p, s = S.local(pw), S.size[:3]
  d = float(np.linalg.norm(p - nearest(p, s, True)))
  return -d if ((p / s) ** 2).sum() <= 1.0 else d


def support(S, d):
  sl = S.size[:3] * (S.R.T @ np.asarray(d, float))
  return S.world(S.size[:3] * sl / np.linalg.norm(sl))


def project(S, pw):
  return S.world(nearest(S.local(pw), S.size[:3])) if S.kind == ELLIPSOID else _project(S, pw)


def height(S, D):
  D = np.atleast_2d(np.asarray(D, float))
  if S.kind == ELLIPSOID:
    return np.linalg.norm((D @ S.R) * S.size[:3], axis=1) + D @ S.pos
  if S.kind == CAPSULE:
    return S.size[0] + S.size[1] * np.abs(D @ S.R[:, 2]) + D @ S.pos
  return _height(S, D)


C.signed_distance, C.project, C.height = signed_distance, project, height
closest, directional_depth, minimal_depth = C.closest, C.directional_depth, C.minimal_depth
