"""fp64 reference of the constraint parameters and of small constraint problems (numpy only).

It restates the documented MuJoCo rules that turn contacts and joint limits into the Newton
problem -- mj_contactParam, mj_makeImpedance, the regulariser R and the reference acceleration,
in-gap contacts -- and solves the resulting problem exactly by enumerating active sets.  It
shares no code with oracle/oracle.c or csrc/engine_impl.h: tests/test_constraint_params.py
holds the oracle to it, tests/test_gpu_constraint_params.py the engine.

Two analytic scenes (tests/constraint_scenes.py builds the same ones as compiled models):

  ball_plane   a free body with a sphere geom (mass, diagonal inertia at the body origin) over
               a tilted plane: M = diag(m, m, m, I), the contact point and its Jacobian exact;
  limit_pair   a slide and a hinge with an offset point-like mass, each on the world with
               armature: M = diag(m + arm, I_axis + arm), one or two limit rows per joint.

Every function takes `mutate=`: the name of one rule to replace by a plausible wrong one
(MUTANTS).  A test whose inputs make no mutant visible would not notice that rule being wrong.
"""

from __future__ import annotations

import itertools

import numpy as np

MINVAL = 1e-15   # mjMINVAL
MINMU = 1e-5     # mjMINMU
MINIMP = 1e-4    # mjMINIMP
MAXIMP = 0.9999  # mjMAXIMP
MAX_ROWS = 10

CONTACT_MUTANTS = ("priority_reversed", "mix_swapped", "friction_min", "condim_min",
                   "solref_always_mixed", "solref_always_min", "gap_ignored", "ingap_rows_kept",
                   "impratio_ignored", "tran_one_body")
SHARED_MUTANTS = ("no_2h_floor", "k_without_dmax2", "imp_mid_swapped")
LIMIT_MUTANTS = ("limit_sign_flipped", "upper_only_when_both", "jnt_margin_ignored")
MUTANTS = CONTACT_MUTANTS + SHARED_MUTANTS + LIMIT_MUTANTS


# ----------------------------------------------------------------------------- parameters
def mix_params(g1: dict, g2: dict, mutate: str | None = None) -> dict:
  """mj_contactParam for two geoms, each a dict of priority, condim, friction [3], solmix,
  solref [2], solimp [5], margin, gap: the contact's dim, friction mu (both tangents of a
  condim-3 contact use friction[0]), solref, solimp, margin and includemargin."""
  p1, p2 = int(g1["priority"]), int(g2["priority"])
  f1, f2 = np.asarray(g1["friction"], float), np.asarray(g2["friction"], float)
  r1, r2 = np.asarray(g1["solref"], float), np.asarray(g2["solref"], float)
  i1, i2 = np.asarray(g1["solimp"], float), np.asarray(g2["solimp"], float)
  if p1 != p2:
    first = (p1 > p2) != (mutate == "priority_reversed")
    g = g1 if first else g2
    dim, fri = int(g["condim"]), np.asarray(g["friction"], float)
    solref, solimp = np.asarray(g["solref"], float), np.asarray(g["solimp"], float)
  else:
    pick = min if mutate == "condim_min" else max
    dim = pick(int(g1["condim"]), int(g2["condim"]))
    fri = np.minimum(f1, f2) if mutate == "friction_min" else np.maximum(f1, f2)
    s1, s2 = float(g1["solmix"]), float(g2["solmix"])
    if s1 < MINVAL and s2 < MINVAL:
      mix = 0.5
    elif s1 < MINVAL:
      mix = 0.0
    elif s2 < MINVAL:
      mix = 1.0
    else:
      mix = s1 / (s1 + s2)
    if mutate == "mix_swapped":
      mix = 1.0 - mix
    mixed = r1[0] > 0 and r2[0] > 0
    if mutate == "solref_always_mixed":
      mixed = True
    if mutate == "solref_always_min":
      mixed = False
    solref = mix * r1 + (1 - mix) * r2 if mixed else np.minimum(r1, r2)
    solimp = mix * i1 + (1 - mix) * i2
  margin = max(float(g1["margin"]), float(g2["margin"]))
  gap = max(float(g1["gap"]), float(g2["gap"]))
  return dict(dim=dim, mu=max(MINMU, float(fri[0])), solref=solref, solimp=solimp, margin=margin,
              includemargin=margin if mutate == "gap_ignored" else margin - gap)


def impedance(solimp, r: float, mutate: str | None = None) -> float:
  """mj_makeImpedance's d(r) for the distance r = |pos - margin|."""
  dmin, dmax, width, mid, power = (float(x) for x in solimp)
  dmin = min(MAXIMP, max(MINIMP, dmin))
  dmax = min(MAXIMP, max(MINIMP, dmax))
  width = max(0.0, width)
  mid = min(MAXIMP, max(MINIMP, mid))
  power = max(1.0, power)
  if dmin == dmax or width <= MINVAL:
    return 0.5 * (dmin + dmax)
  x = abs(r) / width
  if x >= 1.0:
    return dmax
  if x <= 0.0:
    return dmin
  if power == 1.0:
    y = x
  elif (x <= mid) != (mutate == "imp_mid_swapped"):
    y = x ** power / mid ** (power - 1.0)
  else:
    y = 1.0 - (1.0 - x) ** power / (1.0 - mid) ** (power - 1.0)
  return dmin + y * (dmax - dmin)


def kb(solref, solimp, h: float, mutate: str | None = None):
  """Stiffness K and damping B of the reference acceleration: (timeconst, dampratio) with the
  timeconst floored at 2 h, or the direct form (-K, -B) for solref[0] <= 0."""
  dmax = min(MAXIMP, max(MINIMP, float(solimp[1])))
  d2 = 1.0 if mutate == "k_without_dmax2" else dmax * dmax
  if solref[0] > 0:
    tc = float(solref[0]) if mutate == "no_2h_floor" else max(float(solref[0]), 2.0 * h)
    dr = float(solref[1])
    return 1.0 / (d2 * tc * tc * dr * dr), 2.0 / (dmax * tc)
  return -float(solref[0]) / d2, -float(solref[1]) / dmax


def make_row(pos, margin, diag, solref, solimp, h, jv, mutate=None):
  """(D, aref) of one row: R = max(MINVAL, (1 - d) diag / d), aref = -B J v - K d (pos - margin)."""
  d = impedance(solimp, pos - margin, mutate)
  K, B = kb(solref, solimp, h, mutate)
  R = max(MINVAL, (1.0 - d) * diag / d)
  return 1.0 / R, -B * jv - K * d * (pos - margin)


# ----------------------------------------------------------------------------- the solver
def solve_rows(M, a0, J, D, aref):
  """The exact minimiser of 1/2 (a - a0)' M (a - a0) + sum_i 1/2 D_i min(0, J_i a - aref_i)^2
  and the number of consistent active sets (1 for a well-posed problem; asserted): for every
  set S of rows, (M + J_S' D_S J_S) a = M a0 + J_S' D_S aref_S; S is consistent when exactly its
  rows have a negative residual at that a.  The system is solved in its dual form, which stays
  well conditioned for large D: with f_S = -D_S (J_S a - aref_S) the rows' forces,
  (J_S M^-1 J_S' + 1 / D_S) f_S = aref_S - J_S a0 and a = a0 + M^-1 J_S' f_S; the active rows'
  residuals are -f_S / D_S."""
  M, a0 = np.asarray(M, float), np.asarray(a0, float)
  J = np.asarray(J, float).reshape(-1, a0.size)
  D, aref = np.asarray(D, float), np.asarray(aref, float)
  n = J.shape[0]
  assert n <= MAX_ROWS, f"{n} rows: the enumeration handles at most {MAX_ROWS}"
  Minv = np.linalg.inv(M)
  found = []
  for bits in itertools.product((False, True), repeat=n):
    S = np.array(bits, bool)
    Js = J[S]
    try:
      f = np.linalg.solve(Js @ Minv @ Js.T + np.diag(1.0 / D[S]), aref[S] - Js @ a0) if S.any() else np.zeros(0)
    except np.linalg.LinAlgError:  # dependent rows without regularisation: no solution of this set
      continue
    a = a0 + Minv @ (Js.T @ f)
    res = J @ a - aref
    res[S] = -f / D[S]
    if np.array_equal(res < 0.0, S):
      found.append(a)
  assert len(found) == 1, f"{len(found)} consistent active sets of {n} rows"
  return found[0], len(found)


def row_forces(J, D, aref, a):
  J = np.asarray(J, float).reshape(-1, np.size(a))
  return -np.asarray(D, float) * np.minimum(0.0, J @ a - np.asarray(aref, float))


def decode(force, dim, mu):
  """A contact's force in its frame from its rows' forces: (normal, tangent 1, tangent 2)."""
  f = np.asarray(force, float)
  if f.size == 0:
    return np.zeros(3)
  if dim == 1:
    return np.array([f[0], 0.0, 0.0])
  return np.array([f.sum(), mu * (f[0] - f[1]), mu * (f[2] - f[3])])


# ----------------------------------------------------------------------------- small algebra
def quat_mat(q):
  w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
  return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_mul(a, b):
  w1, x1, y1, z1 = a
  w2, x2, y2, z2 = b
  return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                   w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def check_frame(frame, normal, tol=1e-6):
  """The one output a reference takes from the code under test: a contact frame (rows n, t1,
  t2), used only if orthonormal, right-handed and with the exact normal first.  Any such
  tangent pair spans a valid friction pyramid."""
  F = np.asarray(frame, float).reshape(3, 3)
  assert np.abs(F @ F.T - np.eye(3)).max() < tol, "contact frame is not orthonormal"
  assert np.abs(np.cross(F[0], F[1]) - F[2]).max() < tol, "contact frame is not right-handed"
  assert np.abs(F[0] - normal).max() < tol, "contact frame's first axis is not the exact normal"
  return F


def _finish(out, h, mutate):
  a, nsets = solve_rows(out["M"], out["a0"], out["J"], out["D"], out["aref"])
  f = row_forces(out["J"], out["D"], out["aref"], a)
  out.update(qacc=a, efc_force=f, qfrc_constraint=out["J"].T @ f if f.size else np.zeros(a.size),
             nefc=int(f.size), nsets=nsets)
  return out


# ----------------------------------------------------------------------------- ball_plane
def ball_plane(scene: dict, plane: dict, ball: dict, q, v, frame=None, mutate=None) -> dict:
  """One world of the ball_plane scene.  `scene`: mass, inertia [3] (body axes, at the body
  origin = the sphere's centre), radius, plane_normal, plane_pos, gravity, h, impratio.
  `plane`, `ball`: the geoms' parameter dicts (mix_params).  q [7], v [6]: the free joint's
  state (linear velocity in the world, angular in the body).  `frame`: the contact frame to
  take the tangents from (check_frame), when the contact has friction rows."""
  h, m, r = float(scene["h"]), float(scene["mass"]), float(scene["radius"])
  I = np.asarray(scene["inertia"], float)
  n = np.asarray(scene["plane_normal"], float)
  q, v = np.asarray(q, float), np.asarray(v, float)
  c, Rb, om = q[:3], quat_mat(q[3:7]), v[3:6]
  M = np.diag([m, m, m, *I])
  a0 = np.concatenate([np.asarray(scene["gravity"], float), -np.cross(om, I * om) / I])
  p = mix_params(plane, ball, mutate)
  dist = float(n @ (c - np.asarray(scene["plane_pos"], float))) - r
  out = dict(M=M, a0=a0, dist=dist, ncon=int(dist <= p["margin"]), params=p, dim=p["dim"], mu=p["mu"],
             J=np.zeros((0, 6)), D=np.zeros(0), aref=np.zeros(0), normal=n)
  # rows below includemargin.  (Exactly at dist == margin == includemargin, without a gap, the
  # engine and the oracle keep the rows of the contact their narrowphase admits; the sampled
  # states stay TIE_CLEARANCE away from every such equality.)
  active = dist < p["includemargin"] or (mutate == "ingap_rows_kept" and dist <= p["margin"])
  if out["ncon"]:
    out["pos"] = c - n * (r + 0.5 * dist)
  if out["ncon"] and active:
    rho = out["pos"] - c
    jrow = lambda d: np.concatenate([d, Rb.T @ np.cross(rho, d)])  # d . (v + (Rb om) x rho)
    ar = np.abs(rho)
    # the magnitudes of the terms each entry of a row sums (an fp32 row's error scale)
    jmag = lambda d: np.concatenate([np.abs(d), np.abs(Rb.T) @ np.array(
      [ar[1] * abs(d[2]) + ar[2] * abs(d[1]), ar[2] * abs(d[0]) + ar[0] * abs(d[2]), ar[0] * abs(d[1]) + ar[1] * abs(d[0])])])
    # body_invweight0 of a free body (translation): 1 / mass; the plane's body is the world
    # (the mutant takes geom 1's body alone, on condim-1 contacts: four dependent pyramid rows
    # without regularisation have no unique solution to compare)
    tran = 0.0 if mutate == "tran_one_body" and p["dim"] == 1 else 1.0 / m
    mu = p["mu"]
    if p["dim"] == 1:
      rows, diag, dirs = [jrow(n)], tran, [n]
    else:
      assert p["dim"] == 3
      F = check_frame(frame, n)
      dirs = [n + s * mu * F[k] for k in (1, 2) for s in (1.0, -1.0)]
      rows = [jrow(d) for d in dirs]
      diag = (tran + mu * mu * tran) / (1.0 if mutate == "impratio_ignored" else float(scene["impratio"]))
    J = np.array(rows)
    Da = [make_row(dist, p["includemargin"], diag, p["solref"], p["solimp"], h, float(Jr @ v), mutate)
          for Jr in J]
    out.update(J=J, D=np.array([x[0] for x in Da]), aref=np.array([x[1] for x in Da]),
               Jmag=np.array([jmag(d) for d in dirs]))
  out.setdefault("Jmag", np.zeros((0, 6)))
  _finish(out, h, mutate)
  out["contact_force"] = decode(out["efc_force"], p["dim"], p["mu"])
  # semi-implicit Euler (no damping, no actuator: implicitfast reduces to it)
  vn = v + h * out["qacc"]
  th = np.linalg.norm(vn[3:6]) * h
  dq = np.array([1.0, 0.0, 0.0, 0.0]) if th < 1e-300 else \
    np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * vn[3:6] * h / th])
  qn = quat_mul(q[3:7], dq)
  out.update(qvel=vn, qpos=np.concatenate([c + h * vn[:3], qn / np.linalg.norm(qn)]))
  return out


# ----------------------------------------------------------------------------- limit_pair
def limit_pair(scene: dict, joints: list, q, v, mutate=None) -> dict:
  """One world of the limit_pair scene.  `scene`: h, gravity, and per joint (slide first, then
  hinge) axis, mass, armature, com (the point-like mass's offset from the joint anchor at
  q = 0; the hinge only) and sphere_inertia (2/5 m r^2 of the small sphere carrying the mass).
  `joints`: per joint a dict of range [2], margin, solref [2], solimp [5]."""
  h, g = float(scene["h"]), np.asarray(scene["gravity"], float)
  q, v = np.asarray(q, float), np.asarray(v, float)
  sl, hi = scene["slide"], scene["hinge"]
  us, uh = np.asarray(sl["axis"], float), np.asarray(hi["axis"], float)
  Ms = sl["mass"] + sl["armature"]
  rho0 = np.asarray(hi["com"], float)
  perp = rho0 - uh * (uh @ rho0)
  Mh = hi["sphere_inertia"] + hi["mass"] * float(perp @ perp) + hi["armature"]
  # the hinge's mass at angle q: Rodrigues rotation of its offset about the axis
  cq, sq = np.cos(q[1]), np.sin(q[1])
  rho = rho0 * cq + np.cross(uh, rho0) * sq + uh * (uh @ rho0) * (1 - cq)
  a0 = np.array([sl["mass"] * float(us @ g) / Ms, float(uh @ np.cross(rho, hi["mass"] * g)) / Mh])
  M = np.diag([Ms, Mh])
  J, D, aref, sides = [], [], [], []
  for k, jp in enumerate(joints):
    margin = 0.0 if mutate == "jnt_margin_ignored" else float(jp["margin"])
    lower, upper = q[k] - jp["range"][0], jp["range"][1] - q[k]
    act = [(lower, 1.0)] if lower < margin else []
    if upper < margin:
      act = [(upper, -1.0)] if (act and mutate == "upper_only_when_both") else act + [(upper, -1.0)]
    for dist, sign in act:
      if mutate == "limit_sign_flipped":
        sign = -sign
      Jr = np.zeros(2)
      Jr[k] = sign
      d, ar = make_row(dist, margin, 1.0 / M[k, k], jp["solref"], jp["solimp"], h, float(Jr @ v), mutate)
      J.append(Jr); D.append(d); aref.append(ar); sides.append((k, sign))
  out = dict(M=M, a0=a0, J=np.array(J).reshape(-1, 2), D=np.array(D), aref=np.array(aref), sides=sides,
             ncon=0)
  out["Jmag"] = np.abs(out["J"])
  _finish(out, h, mutate)
  vn = v + h * out["qacc"]
  out.update(qvel=vn, qpos=q + h * vn)
  return out
