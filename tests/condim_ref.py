"""fp64 reference of pyramidal contacts with torsional and rolling friction (numpy only).

It restates MuJoCo's documented rule for contacts of dimension 4 and 6 in the project's reading
and solves each world exactly by active-set enumeration (constraint_ref.solve_rows: a condim-6
contact is exactly its MAX_ROWS = 10).  It shares no code with csrc/engine_impl.h or the oracle
(which does not know condim > 3): tests/test_condim.py checks the reference itself,
tests/test_gpu_condim.py holds the engine to it.

The rule.  The contact's friction is the 5-vector mu = (f0, f0, f1, f2, f2) of the selected
(priority) or per-component-maximum 3-vector geom_friction, every component floored at MINMU.
A contact of dimension dim has 2 (dim - 1) rows, ordered as pairs k = 0 .. dim - 2 of
J_n +/- mu_k J_k: J_0, J_1 the relative linear velocity (body 2 minus body 1) at the contact
point along the two tangents, J_2 the relative angular velocity along the normal, J_3, J_4 the
relative angular velocity along the two tangents.  Pair k's diagonal approximation is
(tran + mu_k^2 (k < 2 ? tran : rot)) / impratio with tran / rot the sums of the two bodies'
body_invweight0[0] / [1]; impedance, K, B, margin and the in-gap rule are per contact
(constraint_ref.make_row).  The wrench in the contact frame: normal force = the sum of all rows,
component k + 1 = mu_k (f_2k - f_2k+1): (normal, tangent 1, tangent 2 | torsional, rolling 1,
rolling 2).

A world is one contact between two bodies, each None (the world body) or one of
  free_body(...)   mass, diagonal inertia at the body origin; q [7], dofs [d, d + 6)
  hinge_body(...)  one hinge on the world: anchor, unit axis, a point-like sphere mass at an offset
which give the rows of a point's linear and of the angular velocity and the body's invweights.

`mutate=` replaces one rule by a plausible wrong one (MUTANTS).
"""

from __future__ import annotations

import numpy as np

import constraint_ref as cr
from constraint_ref import MINMU, check_frame, make_row, quat_mat, quat_mul, row_forces, solve_rows

MUTANTS = ("torsion_uses_f0", "rolling_uses_torsion", "rot_weight_is_tran", "rot_rows_body2_only",
           "rot_sign_body1_kept", "torque_unscaled", "four_rows_only", "minmu_tangent_only")


def friction5(g1: dict, g2: dict, mutate: str | None = None) -> np.ndarray:
  """(f0, f0, f1, f2, f2) of the geom with the higher priority, or the per-component maximum."""
  p1, p2 = int(g1["priority"]), int(g2["priority"])
  f1, f2 = np.asarray(g1["friction"], float), np.asarray(g2["friction"], float)
  f = (f1 if p1 > p2 else f2) if p1 != p2 else np.maximum(f1, f2)
  mu = np.array([f[0], f[0], f[1], f[2], f[2]])
  if mutate == "torsion_uses_f0":
    mu[2] = f[0]
  if mutate == "rolling_uses_torsion":
    mu[3:] = f[1]
  if mutate == "minmu_tangent_only":
    mu[:2] = np.maximum(MINMU, mu[:2])
    return mu
  return np.maximum(MINMU, mu)


class _Body:
  nv = 0

  def lin(self, p, d):
    """Row of d . (velocity of the body's point at p)."""
    raise NotImplementedError

  def ang(self, d):
    """Row of d . (the body's angular velocity)."""
    raise NotImplementedError


class free_body(_Body):
  def __init__(self, mass, inertia, q, dof0, nv):
    self.m, self.I = float(mass), np.asarray(inertia, float)
    self.c, self.R = np.asarray(q[:3], float), quat_mat(q[3:7])
    self.d0, self.nv = dof0, nv
    self.tran, self.rot = 1.0 / self.m, float(np.mean(1.0 / self.I))

  def _row(self, a, b):
    r = np.zeros(self.nv)
    r[self.d0:self.d0 + 3], r[self.d0 + 3:self.d0 + 6] = a, b
    return r

  def lin(self, p, d):  # d . (v + (R om) x rho) = d . v + om . R' (rho x d)
    return self._row(d, self.R.T @ np.cross(p - self.c, d))

  def ang(self, d):
    return self._row(np.zeros(3), self.R.T @ d)

  def lin_mag(self, p, d):
    a = np.abs(p - self.c)
    d = np.abs(d)
    x = np.array([a[1] * d[2] + a[2] * d[1], a[2] * d[0] + a[0] * d[2], a[0] * d[1] + a[1] * d[0]])
    return self._row(d, np.abs(self.R.T) @ x)

  def ang_mag(self, d):
    return self._row(np.zeros(3), np.abs(self.R.T) @ np.abs(d))

  def mass_matrix(self):
    return np.diag([self.m] * 3 + list(self.I))

  def a0(self, v, gravity):
    om = v[self.d0 + 3:self.d0 + 6]
    return np.concatenate([np.asarray(gravity, float), -np.cross(om, self.I * om) / self.I])


class hinge_body(_Body):
  """A hinge on the world at `anchor` about the unit `axis`, carrying a small sphere (mass,
  sphere_inertia = 2/5 m r^2) whose centre is at anchor + Rot(axis, q) com; armature on the dof."""

  def __init__(self, anchor, axis, mass, sphere_inertia, armature, com, q, dof0=0, nv=1):
    self.p0, self.u = np.asarray(anchor, float), np.asarray(axis, float)
    self.m, self.d0, self.nv = float(mass), dof0, nv
    rho0 = np.asarray(com, float)
    perp = rho0 - self.u * (self.u @ rho0)
    self.M = float(sphere_inertia) + self.m * float(perp @ perp) + float(armature)
    cq, sq = np.cos(q), np.sin(q)
    self.rho = rho0 * cq + np.cross(self.u, rho0) * sq + self.u * (self.u @ rho0) * (1 - cq)
    self.c = self.p0 + self.rho
    # body_invweight0 at the inertial frame (the sphere's centre): trace(J M^-1 J') / 3
    self.tran = float(np.sum(np.cross(self.u, rho0) ** 2)) / (3.0 * self.M)
    self.rot = 1.0 / (3.0 * self.M)

  def _row(self, x):
    r = np.zeros(self.nv)
    r[self.d0] = x
    return r

  def lin(self, p, d):
    return self._row(float(d @ np.cross(self.u, p - self.p0)))

  def ang(self, d):
    return self._row(float(d @ self.u))

  def lin_mag(self, p, d):
    a, u, d = np.abs(p - self.p0), np.abs(self.u), np.abs(d)
    x = np.array([u[1] * a[2] + u[2] * a[1], u[2] * a[0] + u[0] * a[2], u[0] * a[1] + u[1] * a[0]])
    return self._row(float(d @ x))

  def ang_mag(self, d):
    return self._row(float(np.abs(d) @ np.abs(self.u)))

  def mass_matrix(self):
    return np.array([[self.M]])

  def a0(self, v, gravity):
    return np.array([float(self.u @ np.cross(self.rho, self.m * np.asarray(gravity, float))) / self.M])


def _rel(b1, b2, fn, *args):
  """Body 2 minus body 1 (None: the world body, no dofs)."""
  nv = (b2 or b1).nv
  r = np.zeros(nv)
  if b2 is not None:
    r = r + getattr(b2, fn)(*args)
  if b1 is not None:
    r = r - getattr(b1, fn)(*args)
  return r


def _mag(b1, b2, fn, *args):
  nv = (b2 or b1).nv
  r = np.zeros(nv)
  for b in (b1, b2):
    if b is not None:
      r = r + getattr(b, fn + "_mag")(*args)
  return r


def contact_world(h, impratio, gravity, bodies, v, g1, g2, b1, b2, dist, pos, normal, frame=None,
                  mutate=None) -> dict:
  """One world: `bodies` in dof order (their blocks make M and a0), qvel `v`, and one candidate
  contact between geoms g1 / g2 (constraint_ref.mix_params dicts) of bodies b1 / b2 at distance
  `dist`, position `pos`, unit `normal` (from geom 1 to geom 2).  `frame`: the contact frame to
  take the tangents from (check_frame), when the contact has friction rows."""
  v = np.asarray(v, float)
  nv = v.size
  M, a0 = np.zeros((nv, nv)), np.zeros(nv)
  for b in bodies:
    k = b.mass_matrix().shape[0]
    M[b.d0:b.d0 + k, b.d0:b.d0 + k] = b.mass_matrix()
    a0[b.d0:b.d0 + k] = b.a0(v, gravity)
  p = cr.mix_params(g1, g2)
  mu = friction5(g1, g2, mutate)
  dim = p["dim"]
  n = np.asarray(normal, float)
  out = dict(M=M, a0=a0, dist=float(dist), ncon=int(dist <= p["margin"]), params=p, dim=dim, mu=mu,
             J=np.zeros((0, nv)), D=np.zeros(0), aref=np.zeros(0), Jmag=np.zeros((0, nv)), normal=n)
  if out["ncon"]:
    out["pos"] = np.asarray(pos, float)
  npair = 0
  if out["ncon"] and dist < p["includemargin"]:
    tran = sum(b.tran for b in (b1, b2) if b is not None)
    rot = sum(b.rot for b in (b1, b2) if b is not None)
    if mutate == "rot_weight_is_tran":
      rot = tran
    jn, jn_mag = _rel(b1, b2, "lin", pos, n), _mag(b1, b2, "lin", pos, n)
    rows, mags, diags = [], [], []
    if dim == 1:
      rows, mags, diags = [jn], [jn_mag], [tran]
    else:
      F = check_frame(frame, n)
      npair = 2 if mutate == "four_rows_only" else dim - 1
      axes = (F[1], F[2], F[0], F[1], F[2])
      for k in range(npair):
        if k < 2:
          jk, jk_mag = _rel(b1, b2, "lin", pos, axes[k]), _mag(b1, b2, "lin", pos, axes[k])
        else:
          if mutate == "rot_rows_body2_only":
            jk = _rel(None, b2, "ang", axes[k]) if b2 is not None else np.zeros(nv)
          elif mutate == "rot_sign_body1_kept":
            jk = _rel(None, b2, "ang", axes[k]) if b2 is not None else np.zeros(nv)
            if b1 is not None:
              jk = jk + b1.ang(axes[k])
          else:
            jk = _rel(b1, b2, "ang", axes[k])
          jk_mag = _mag(b1, b2, "ang", axes[k])
        for s in (1.0, -1.0):
          rows.append(jn + s * mu[k] * jk)
          mags.append(jn_mag + mu[k] * jk_mag)
          diags.append((tran + mu[k] ** 2 * (tran if k < 2 else rot)) / float(impratio))
    J = np.array(rows)
    Da = [make_row(dist, p["includemargin"], dg, p["solref"], p["solimp"], h, float(Jr @ v))
          for Jr, dg in zip(J, diags)]
    out.update(J=J, D=np.array([x[0] for x in Da]), aref=np.array([x[1] for x in Da]), Jmag=np.array(mags))
  a, nsets = solve_rows(out["M"], out["a0"], out["J"], out["D"], out["aref"])
  f = row_forces(out["J"], out["D"], out["aref"], a)
  out.update(qacc=a, efc_force=f, nefc=int(f.size), nsets=nsets,
             qfrc_constraint=out["J"].T @ f if f.size else np.zeros(nv))
  force, torque = decode(f, dim, mu, mutate)
  out.update(contact_force=force, contact_torque=torque)
  return out


def decode(f, dim, mu, mutate=None):
  """(force [3], torque [3]) of a contact in its frame from its rows' forces."""
  f = np.asarray(f, float)
  force, torque = np.zeros(3), np.zeros(3)
  if f.size == 0:
    return force, torque
  if dim == 1:
    force[0] = f[0]
    return force, torque
  force[0] = f.sum()
  for k in range(f.size // 2):
    x = mu[k] * (f[2 * k] - f[2 * k + 1])
    if k < 2:
      force[1 + k] = x
    else:
      torque[k - 2] = (f[2 * k] - f[2 * k + 1]) if mutate == "torque_unscaled" else x
  return force, torque


def integrate_free(q, v, qacc, h):
  """Semi-implicit Euler of a free joint (linear velocity in the world, angular in the body)."""
  vn = v + h * qacc
  th = np.linalg.norm(vn[3:6]) * h
  dq = np.array([1.0, 0.0, 0.0, 0.0]) if th < 1e-300 else \
    np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * vn[3:6] * h / th])
  qn = quat_mul(q[3:7], dq)
  return np.concatenate([q[:3] + h * vn[:3], qn / np.linalg.norm(qn)]), vn
