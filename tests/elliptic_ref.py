"""fp64 reference of contacts with elliptic friction cones (numpy only).

It restates MuJoCo's elliptic cone in the project's reading ("Elliptic
friction cones"; MuJoCo documentation, "Computation": friction cones, mj_makeImpedance,
mj_constraintUpdate) and minimises the resulting convex, C1 cost exactly.  It shares no code with
csrc/engine_impl.h or the oracle (which never learns about cones): tests/test_elliptic.py checks
the reference itself, tests/test_gpu_elliptic.py holds the engine to it.  Bodies, row magnitudes,
friction5 and make_row's parts come from condim_ref / constraint_ref.

The rule.  A contact of dimension dim in {3, 4, 6} has dim rows: J_n (relative linear velocity at
the contact point along the normal, body 2 minus body 1), J_t1, J_t2 (along the frame's tangents),
then the relative angular velocity about the normal and about the two tangents.  friction =
(f0, f0, f1, f2, f2), floored at MINMU.  Impedance imp, K, B, margin and the in-gap rule are per
contact from dist; R_0 = max(MINVAL, (1 - imp) / imp tran), R_1 = R_0 / impratio, R_j = R_1 f0^2 /
friction[j-1]^2, D = 1 / R, mu = f0 / sqrt(impratio); aref_0 = -B J_n v - K imp (dist - margin),
aref_j = -B J_j v.  With jar = J x - aref, s = (mu, friction[:dim-1]), U = s o jar, N = U_0,
T = |U_1..|, the cost is 1/2 (D_0 / mu^2) dist(U, {N >= mu T})^2:
  top     N >= mu T, or T <= 0 and N >= 0: nothing
  bottom  mu N + T <= 0, or T <= 0 and N < 0: 1/2 sum D_j jar_j^2, f_j = -D_j jar_j
  middle  D_m = D_0 / (mu^2 (1 + mu^2)): 1/2 D_m (N - mu T)^2, f_0 = -D_m (N - mu T) mu,
          f_j = -f_0 / T U_j friction[j-1], Hessian D_m diag(s) C diag(s) with C_00 = 1,
          C_0j = -mu U_j / T, C_jk = mu N U_j U_k / T^3 + (mu^2 - mu N / T) delta_jk
The wrench in the contact frame is the row forces: force (f_0, f_1, f_2), torque (f_3, f_4, f_5).
Every other row (a limit, an equality pair's, a condim-1 contact's) is a one-sided half-quadratic.

`mutate=` replaces one rule by a plausible wrong one (MUTANTS).
"""

from __future__ import annotations

import numpy as np

import constraint_ref as cr
from condim_ref import _mag, _rel, friction5
from constraint_ref import MINVAL, check_frame

MUTANTS = ("friction_rows_r0", "mu_without_impratio", "r_unscaled", "friction_aref_pos",
           "middle_is_bottom", "s_on_forces_only", "wrench_pyramidal", "pyramid_row_count")
TOP, BOTTOM, MIDDLE = 0, 1, 2


class slide3_body:
  """A point-like body on three world-aligned slides (dofs d0 .. d0 + 2): M = m I."""

  def __init__(self, mass, c, dof0=0, nv=3):
    self.m, self.c, self.d0, self.nv = float(mass), np.asarray(c, float), dof0, nv
    self.tran, self.rot = 1.0 / self.m, 0.0

  def _row(self, a):
    r = np.zeros(self.nv)
    r[self.d0:self.d0 + 3] = a
    return r

  def lin(self, p, d):
    return self._row(d)

  def ang(self, d):
    return self._row(np.zeros(3))

  def lin_mag(self, p, d):
    return self._row(np.abs(d))

  def ang_mag(self, d):
    return self._row(np.zeros(3))

  def mass_matrix(self):
    return self.m * np.eye(3)

  def a0(self, v, gravity):
    return np.asarray(gravity, float).copy()


# ----------------------------------------------------------------------------- one contact's cost
def zone_of(N, T, mu):
  if T <= 0.0:
    return TOP if N >= 0.0 else BOTTOM
  if N >= mu * T:
    return TOP
  if mu * N + T <= 0.0:
    return BOTTOM
  return MIDDLE


def cone_eval(jar, D, mu, fr, mutate=None):
  """(zone, cost, forces [dim], Hessian [dim, dim] in jar) of one elliptic contact."""
  jar, D, fr = np.asarray(jar, float), np.asarray(D, float), np.asarray(fr, float)
  dim = jar.size
  s = np.concatenate([[mu], fr[:dim - 1]])
  su = np.concatenate([[mu], np.ones(dim - 1)]) if mutate == "s_on_forces_only" else s
  U = su * jar
  N, T = float(U[0]), float(np.linalg.norm(U[1:]))
  z = zone_of(N, T, mu)
  if z == MIDDLE and mutate == "middle_is_bottom":
    z = BOTTOM
  if z == TOP:
    return z, 0.0, np.zeros(dim), np.zeros((dim, dim))
  if z == BOTTOM:
    return z, 0.5 * float(D @ (jar * jar)), -D * jar, np.diag(D)
  Dm = D[0] / (mu * mu * (1.0 + mu * mu))
  f = np.zeros(dim)
  f[0] = -Dm * (N - mu * T) * mu
  f[1:] = -f[0] / T * U[1:] * su[1:]
  C = np.zeros((dim, dim))
  C[0, 0] = 1.0
  C[0, 1:] = C[1:, 0] = -mu * U[1:] / T
  C[1:, 1:] = mu * N * np.outer(U[1:], U[1:]) / T ** 3 + (mu * mu - mu * N / T) * np.eye(dim - 1)
  return z, 0.5 * Dm * (N - mu * T) ** 2, f, Dm * (su[:, None] * C * su[None, :])


def _group_eval(g, jar, mutate):
  if g["kind"] == "cone":
    return cone_eval(jar, g["D"], g["mu"], g["fr"], mutate)
  act = jar < 0.0
  return (BOTTOM if act.any() else TOP, 0.5 * float(g["D"][act] @ (jar[act] ** 2)),
          -g["D"] * np.minimum(jar, 0.0), np.diag(g["D"] * act))


# ----------------------------------------------------------------------------- rows
def ordinary(J, D, aref, Jmag=None):
  """A group of one-sided half-quadratic rows."""
  J = np.atleast_2d(np.asarray(J, float))
  return dict(kind="ord", J=J, D=np.atleast_1d(np.asarray(D, float)), aref=np.atleast_1d(np.asarray(aref, float)),
              Jmag=np.abs(J) if Jmag is None else np.atleast_2d(np.asarray(Jmag, float)))


def contact_group(h, impratio, v, g1, g2, b1, b2, dist, pos, normal, frame=None, mutate=None):
  """The candidate contact's record: ncon (0 / 1), and with rows its group (kind "cone" for a
  contact with friction, "ord" for condim 1).  g1 / g2: constraint_ref.mix_params dicts; b1 / b2:
  condim_ref bodies (None: the world); `frame`: the contact frame to take the tangents from."""
  v = np.asarray(v, float)
  p = cr.mix_params(g1, g2)
  fr = friction5(g1, g2)
  dim = p["dim"]
  n = np.asarray(normal, float)
  out = dict(ncon=int(dist <= p["margin"]), dim=dim, fr=fr, dist=float(dist), params=p, normal=n, group=None,
             pos=np.asarray(pos, float))
  if not (out["ncon"] and dist < p["includemargin"]):
    return out
  tran = sum(b.tran for b in (b1, b2) if b is not None)
  imp = cr.impedance(p["solimp"], dist - p["includemargin"])
  K, B = cr.kb(p["solref"], p["solimp"], h)
  jn, jn_mag = _rel(b1, b2, "lin", pos, n), _mag(b1, b2, "lin", pos, n)
  R0 = max(MINVAL, (1.0 - imp) / imp * tran)
  if dim == 1:
    out["group"] = ordinary(jn, 1.0 / R0, -B * float(jn @ v) - K * imp * (dist - p["includemargin"]), jn_mag)
    return out
  F = check_frame(frame, n)
  axes = (F[0], F[1], F[2], F[0], F[1], F[2])
  rows, mags = [], []
  for j in range(dim):
    kind = "lin" if j < 3 else "ang"
    args = (pos, axes[j]) if j < 3 else (axes[j],)
    rows.append(_rel(b1, b2, kind, *args))
    mags.append(_mag(b1, b2, kind, *args))
  J = np.array(rows)
  f0 = fr[0]
  R1 = R0 if mutate == "friction_rows_r0" else R0 / float(impratio)
  R = np.array([R0] + [R1 if mutate == "r_unscaled" else R1 * f0 * f0 / fr[j - 1] ** 2 for j in range(1, dim)])
  aref = -B * (J @ v)
  aref[0] -= K * imp * (dist - p["includemargin"])
  if mutate == "friction_aref_pos":
    aref[1:] -= K * imp * (dist - p["includemargin"])
  mu = f0 if mutate == "mu_without_impratio" else f0 / np.sqrt(float(impratio))
  out["group"] = dict(kind="cone", J=J, D=1.0 / R, aref=aref, Jmag=np.array(mags), mu=float(mu), fr=fr[:dim - 1].copy())
  return out


# ----------------------------------------------------------------------------- the exact minimiser
def _eval(M, a0, groups, x, mutate, hess=False):
  dx = x - a0
  cost, grad = 0.5 * float(dx @ M @ dx), M @ dx
  H = M.copy() if hess else None
  fs, zs = [], []
  mag = np.abs(M) @ np.abs(dx)
  for g in groups:
    z, c, f, Hc = _group_eval(g, g["J"] @ x - g["aref"], mutate)
    cost += c
    grad = grad - g["J"].T @ f
    mag = mag + np.abs(g["J"]).T @ np.abs(f)
    if hess:
      H += g["J"].T @ Hc @ g["J"]
    fs.append(f)
    zs.append(z)
  return cost, grad, H, fs, zs, mag


def minimise(M, a0, groups, mutate=None, iters=200):
  """The unique minimiser of 1/2 (x - a0)' M (x - a0) + the groups' costs (M > 0, the cost convex
  and C1): damped Newton with an exact line search -- the root of the monotone derivative along
  the step, bisected to rounding.  Accepted only with |M (x - a0) - J' f|_inf at fp64 rounding
  level of the summed terms' magnitudes (per dof, plus 1e-6 of the largest for a dof whose own
  terms vanish).  Returns (x, forces per group, zones, Newton steps)."""
  M, a0 = np.asarray(M, float), np.asarray(a0, float)
  x = a0.copy()
  for it in range(iters):
    cost, grad, H, fs, zs, mag = _eval(M, a0, groups, x, mutate, hess=True)
    if np.all(np.abs(grad) <= 1e-13 * (mag + 1e-6 * mag.max() + 1e-300)) or not np.any(grad):
      break
    step = -np.linalg.solve(H, grad)
    der = lambda a: float(_eval(M, a0, groups, x + a * step, mutate)[1] @ step)
    lo, hi = 0.0, 1.0
    while der(hi) < 0.0 and hi < 1e6:
      lo, hi = hi, 2.0 * hi
    for _ in range(200):
      mid = 0.5 * (lo + hi)
      if mid in (lo, hi):
        break
      lo, hi = (mid, hi) if der(mid) < 0.0 else (lo, mid)
    x = x + 0.5 * (lo + hi) * step
  cost, grad, _, fs, zs, mag = _eval(M, a0, groups, x, mutate)
  ok = bool(np.all(np.abs(grad) <= 1e-9 * (mag + 1e-6 * mag.max() + 1e-300)))
  # (a mutant's cost need not be C1 or convex: its result is whatever the iteration reached)
  assert ok or mutate is not None, \
      f"the minimiser did not converge: gradient {np.abs(grad).max():.3e} of terms {mag.max():.3e}"
  return x, fs, zs, it


def decode(f, dim, fr, mutate=None):
  """(force [3], torque [3]) of a contact in its frame from its rows' forces."""
  force, torque = np.zeros(3), np.zeros(3)
  f = np.asarray(f, float)
  if f.size == 0:
    return force, torque
  if dim == 1:
    force[0] = f[0]
    return force, torque
  if mutate == "s_on_forces_only":
    f = f * np.concatenate([[1.0], fr[:dim - 1]])
  if mutate == "wrench_pyramidal":  # the pyramid's decode applied to the first rows
    force[0] = f.sum()
    pairs = [fr[k] * (f[2 * k] - f[2 * k + 1]) if 2 * k + 1 < f.size else 0.0 for k in range(5)]
    force[1:], torque[:] = pairs[:2], pairs[2:]
    return force, torque
  w = np.zeros(6)
  w[:dim] = f
  return w[:3], w[3:]


def solve_world(M, a0, contacts, extra=(), mutate=None) -> dict:
  """A world: `extra` ordinary groups first (equality | limit order is the caller's), then the
  contacts' groups in contact order.  Per contact: contact_force / contact_torque / zone."""
  groups = list(extra) + [c["group"] for c in contacts if c["group"] is not None]
  M, a0 = np.asarray(M, float), np.asarray(a0, float)
  nv = a0.size
  if groups:
    x, fs, zs, nit = minimise(M, a0, groups, mutate)
  else:
    x, fs, zs, nit = a0.copy(), [], [], 0
  J = np.concatenate([g["J"] for g in groups]) if groups else np.zeros((0, nv))
  f = np.concatenate(fs) if fs else np.zeros(0)
  out = dict(M=M, a0=a0, qacc=x, efc_force=f, J=J, groups=groups, zones=zs, newton=nit,
             Jmag=np.concatenate([g["Jmag"] for g in groups]) if groups else np.zeros((0, nv)),
             D=np.concatenate([g["D"] for g in groups]) if groups else np.zeros(0),
             aref=np.concatenate([g["aref"] for g in groups]) if groups else np.zeros(0),
             qfrc_constraint=J.T @ f if f.size else np.zeros(nv), ncon=sum(c["ncon"] for c in contacts))
  nefc = int(f.size)
  if mutate == "pyramid_row_count":
    nefc += sum(c["dim"] - 2 for c in contacts if c["group"] is not None and c["dim"] > 1)
  out["nefc"] = nefc
  k = len(extra)
  cf, ct, cz = [], [], []
  for c in contacts:
    if not c["ncon"]:
      continue
    if c["group"] is None:
      cf.append(np.zeros(3)); ct.append(np.zeros(3)); cz.append(TOP)
      continue
    a, b = decode(fs[k], c["dim"], c["fr"], mutate)
    cf.append(a); ct.append(b); cz.append(zs[k])
    k += 1
  out.update(contact_force=np.array(cf).reshape(-1, 3), contact_torque=np.array(ct).reshape(-1, 3), contact_zone=cz)
  return out


def contact_world(h, impratio, gravity, bodies, v, g1, g2, b1, b2, dist, pos, normal, frame=None, mutate=None):
  """condim_ref.contact_world's signature: one candidate contact between two bodies."""
  v = np.asarray(v, float)
  nv = v.size
  M, a0 = np.zeros((nv, nv)), np.zeros(nv)
  for b in bodies:
    k = b.mass_matrix().shape[0]
    M[b.d0:b.d0 + k, b.d0:b.d0 + k] = b.mass_matrix()
    a0[b.d0:b.d0 + k] = b.a0(v, gravity)
  c = contact_group(h, impratio, v, g1, g2, b1, b2, dist, pos, normal, frame, mutate)
  out = solve_world(M, a0, [c], mutate=mutate)
  out.update(dist=c["dist"], dim=c["dim"], fr=c["fr"], params=c["params"], normal=c["normal"], pos=c["pos"],
             mu=c["group"]["mu"] if c["group"] is not None and c["group"]["kind"] == "cone" else None)
  return out


# ----------------------------------------------------------------------------- fp32 error scales
def hessian(r: dict) -> np.ndarray:
  """The Newton Hessian at the solution: M + sum J' H_c J, the cone Hessians included."""
  return _eval(r["M"], r["a0"], r["groups"], r["qacc"], None, hess=True)[2]


def force_bounds(r: dict, ab):
  """Per row (first, mag): `first` the force's sensitivity to jar -- |H_c| in the middle zone, D_j
  in the bottom zone, for an ordinary row and around a top-zone contact -- times the rows' jar
  error |J| ab; `mag` the same sensitivity times the magnitudes |aref| + |J| |a| of the terms a
  jar sums (x c eps32: the fp32 rounding part, tests/test_gpu_constraint_params.py)."""
  ab = np.asarray(ab, float)
  first, mag = [], []
  for g in r["groups"]:
    jar_err = g["Jmag"] @ ab
    jar_mag = np.abs(g["aref"]) + g["Jmag"] @ np.abs(r["qacc"])
    z, _, f, Hc = _group_eval(g, g["J"] @ r["qacc"] - g["aref"], None)
    S = np.abs(Hc) if (g["kind"] == "cone" and z == MIDDLE) else np.diag(g["D"])
    first.append(S @ jar_err)
    mag.append(S @ jar_mag)
  cat = lambda x: np.concatenate(x) if x else np.zeros(0)
  return cat(first), cat(mag)
