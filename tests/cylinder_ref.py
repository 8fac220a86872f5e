"""Independent fp64 geometry of the cylinder narrowphase tests (numpy only; no engine, no oracle).
A cylinder is narrowphase_ref's Shape of kind CYLINDER: size (r, h), axis = column 2.  Closed-form
supports and projections give the exact distance of separated convex shapes (alternating
projections) and the directional depth of overlapping ones, with its minimum over n."""

import numpy as np

import narrowphase_ref as R
from narrowphase_ref import BOX, CAPSULE, PLANE, SPHERE

CYLINDER = 5


def sd_cylinder(p, r, h):
  dr, dz = np.hypot(p[0], p[1]) - r, abs(p[2]) - h
  return float(np.hypot(max(dr, 0.0), max(dz, 0.0)) + min(max(dr, dz), 0.0))


def signed_distance(S, pw):
  return sd_cylinder(S.local(pw), *S.size[:2]) if S.kind == CYLINDER else R.signed_distance(S, pw)


def support(S, d):
  """A farthest point of a cylinder or box along the world direction d."""
  l = S.R.T @ np.asarray(d, float)
  if S.kind == CYLINDER:
    rad = l[:2] * (S.size[0] / np.hypot(l[0], l[1])) if np.hypot(l[0], l[1]) > 0 else np.zeros(2)
    return S.world(np.array([rad[0], rad[1], np.copysign(S.size[1], l[2])]))
  return S.world(np.copysign(S.size[:3], l))


def project(S, pw):
  """The point of the solid nearest the world point pw (pw itself when inside)."""
  p = S.local(pw)
  if S.kind == PLANE:
    q = np.array([p[0], p[1], min(p[2], 0.0)])
  elif S.kind in (SPHERE, CAPSULE):
    c = np.array([0.0, 0.0, np.clip(p[2], -S.size[1], S.size[1]) if S.kind == CAPSULE else 0.0])
    d = np.linalg.norm(p - c)
    q = p if d <= S.size[0] else c + (p - c) * (S.size[0] / d)
  elif S.kind == CYLINDER:
    rho = np.hypot(p[0], p[1])
    k = min(1.0, S.size[0] / rho) if rho > 0 else 1.0
    q = np.array([p[0] * k, p[1] * k, np.clip(p[2], -S.size[1], S.size[1])])
  else:
    assert S.kind == BOX
    q = np.clip(p, -S.size[:3], S.size[:3])
  return S.world(q)


def closest(A, B, tol=1e-12, iters=200000):
  """(distance, point of A, point of B, unit direction A to B); distance 0 when they touch or overlap."""
  y = project(B, A.pos if A.kind != PLANE else B.pos)
  last = np.inf
  for _ in range(iters):
    x = project(A, y)
    y = project(B, x)
    d = float(np.linalg.norm(y - x))
    if last - d <= tol * 1e-2 or d <= tol:
      break
    last = d
  if d <= 1e-10:
    return 0.0, x, y, np.zeros(3)
  return d, x, y, (y - x) / d


def height(S, D):
  """Support heights max over a cylinder or box of d . x for the world directions D (N, 3)."""
  D = np.atleast_2d(np.asarray(D, float))
  L = D @ S.R
  if S.kind == CYLINDER:
    return S.size[0] * np.hypot(L[:, 0], L[:, 1]) + S.size[1] * np.abs(L[:, 2]) + D @ S.pos
  assert S.kind == BOX
  return np.abs(L) @ S.size[:3] + D @ S.pos


def directional_depth(A, B, n):
  """h_A(n) + h_B(-n) - n . (c_B - c_A): how far B has to move along n to leave A.  n: (3) or (N, 3)."""
  n = np.asarray(n, float)
  if A.kind == PLANE:  # the half-space below the plane: only its own normal bounds it
    out = float(A.R[:, 2] @ A.pos) + height(B, -np.atleast_2d(n))
  else:
    out = height(A, n) + height(B, -np.atleast_2d(n))
  return float(out[0]) if n.ndim == 1 else out


_i = np.arange(4096) + 0.5  # 4,096 directions on the unit sphere (Fibonacci lattice)
_z, _phi = 1.0 - 2.0 * _i / 4096, np.pi * (1.0 + 5.0 ** 0.5) * _i
GRID = np.stack([np.sqrt(1.0 - _z * _z) * np.cos(_phi), np.sqrt(1.0 - _z * _z) * np.sin(_phi), _z], axis=1)


def minimal_depth(A, B):
  """(depth, direction): the least directional depth over GRID, refined once on a 41 x 41 patch."""
  d = directional_depth(A, B, GRID)
  n0 = GRID[int(np.argmin(d))]
  t = np.cross(n0, [1.0, 0.0, 0.0] if abs(n0[0]) < 0.9 else [0.0, 1.0, 0.0])
  t /= np.linalg.norm(t)
  b = np.cross(n0, t)
  u = np.linspace(-0.04, 0.04, 41)
  cand = n0[None, None, :] + u[:, None, None] * t + u[None, :, None] * b
  cand = (cand / np.linalg.norm(cand, axis=2, keepdims=True)).reshape(-1, 3)
  dd = directional_depth(A, B, cand)
  k = int(np.argmin(dd))
  return (float(dd[k]), cand[k]) if dd[k] < d.min() else (float(d.min()), n0)
