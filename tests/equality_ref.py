"""fp64 reference of joint equality constraints (numpy only; test infrastructure).

It restates MuJoCo's mjEQ_JOINT rule and solves the resulting constraint problem exactly.  It
shares no code with csrc/engine_impl.h or oracle/oracle.c (the oracle ignores equalities); the
impedance, the stiffness / damping rule, the row (D, aref) of limits and contacts and the
enumeration of active sets are tests/constraint_ref.py's.

For equality e with joints j1, optional j2 (hinge or slide) and polycoef c[0..4]:

  d = qpos[j2] - qpos0[j2],  poly(d) = c0 + c1 d + c2 d^2 + c3 d^3 + c4 d^4
  pos = qpos[j1] - qpos0[j1] - poly(d),  J[dof1] = 1,  J[dof2] = -(c1 + 2 c2 d + 3 c3 d^2 + 4 c4 d^3)
  without j2: pos = qpos[j1] - qpos0[j1] - c0, J[dof1] = 1
  margin = 0, diagApprox = dof_invweight0[dof1] (+ dof_invweight0[dof2])
  imp, K, B from eq_solimp / eq_solref; R = max(MINVAL, (1 - imp) / imp diag), D = 1 / R,
  aref = -B (J qvel) - K imp pos; the row is always active: its cost 1/2 D (J x - aref)^2 counts
  on both sides.

`solve` minimises 1/2 (x - a0)' M (x - a0) + sum_eq 1/2 D (J x - aref)^2 + sum_ineq 1/2 D
min(0, J x - aref)^2 exactly: the equality rows belong to every active set, the inequality rows
(limits, contacts) are enumerated.  With `pair=True` every equality row is replaced by the two
opposed one-sided rows (+J, +aref) and (-J, -aref) the engine emits; the minimiser is the same.

`mutate=` names one rule to replace by a plausible wrong one (MUTANTS), in the style of
constraint_ref.MUTANTS: a test whose inputs make no mutant visible would not notice that rule
being wrong.
"""

from __future__ import annotations

import itertools

import numpy as np

import constraint_ref as cr

MUTANTS = ("poly_derivative_dropped", "qpos0_ignored", "data0_ignored", "diag_first_dof_only",
           "second_sign_flipped", "one_sided", "solref_from_joint")


def equality_row(eq: dict, qpos, qpos0, qvel, invweight, h: float, nv: int, mutate: str | None = None) -> dict:
  """The row of one joint equality.  `eq`: qadr1, dof1, qadr2 / dof2 (None: joint1 alone),
  polycoef [5], solref [2], solimp [5], and jnt_solref / jnt_solimp of joint 1 (read by the
  solref_from_joint mutant only).  Returns J [nv], pos, D, aref, diag, imp."""
  c = np.array(eq["polycoef"], float)
  if mutate == "data0_ignored":
    c[0] = 0.0
  q0 = np.zeros_like(np.asarray(qpos0, float)) if mutate == "qpos0_ignored" else np.asarray(qpos0, float)
  J = np.zeros(nv)
  J[eq["dof1"]] = 1.0
  diag = float(invweight[eq["dof1"]])
  if eq.get("dof2") is not None:
    d = float(qpos[eq["qadr2"]] - q0[eq["qadr2"]])
    poly = c[0] + c[1] * d + c[2] * d ** 2 + c[3] * d ** 3 + c[4] * d ** 4
    dpoly = c[1] + 2 * c[2] * d + 3 * c[3] * d ** 2 + 4 * c[4] * d ** 3
    if mutate == "poly_derivative_dropped":
      dpoly = c[1]
    J[eq["dof2"]] = dpoly if mutate == "second_sign_flipped" else -dpoly
    if mutate != "diag_first_dof_only":
      diag += float(invweight[eq["dof2"]])
  else:
    poly = c[0]
  pos = float(qpos[eq["qadr1"]] - q0[eq["qadr1"]]) - poly
  solref, solimp = eq["solref"], eq["solimp"]
  if mutate == "solref_from_joint":
    solref, solimp = eq["jnt_solref"], eq["jnt_solimp"]
  D, aref = cr.make_row(pos, 0.0, diag, solref, solimp, h, float(J @ np.asarray(qvel, float)))
  return dict(J=J, pos=pos, D=D, aref=aref, diag=diag, imp=cr.impedance(solimp, pos))


def solve(M, a0, Je, De, arefe, Ji=None, Di=None, arefi=None, pair: bool = False, mutate: str | None = None):
  """The exact minimiser (module docstring) and the rows' forces.  Returns a dict: qacc, the
  equality forces f_eq (signed: f = -D (J x - aref)), the inequality forces f_ineq (>= 0), the
  active inequality set, and kkt = |M (x - a0) - J' f|_inf.  Solved in the dual form of
  constraint_ref.solve_rows, which stays well conditioned for stiff rows."""
  M, a0 = np.asarray(M, float), np.asarray(a0, float)
  nv = a0.size
  Je = np.asarray(Je, float).reshape(-1, nv)
  De, arefe = np.asarray(De, float).reshape(-1), np.asarray(arefe, float).reshape(-1)
  Ji = np.zeros((0, nv)) if Ji is None else np.asarray(Ji, float).reshape(-1, nv)
  Di = np.zeros(0) if Di is None else np.asarray(Di, float).reshape(-1)
  arefi = np.zeros(0) if arefi is None else np.asarray(arefi, float).reshape(-1)
  ne = Je.shape[0]
  if pair or mutate == "one_sided":
    # the opposed pair (or, for the mutant, its first row alone) as one-sided rows
    rows = [(Je[k], De[k], arefe[k]) for k in range(ne)]
    if pair and mutate != "one_sided":
      rows += [(-Je[k], De[k], -arefe[k]) for k in range(ne)]
    Ji = np.vstack([np.array([r[0] for r in rows]).reshape(-1, nv), Ji])
    Di = np.concatenate([[r[1] for r in rows], Di])
    arefi = np.concatenate([[r[2] for r in rows], arefi])
    Je, De, arefe, nmoved = np.zeros((0, nv)), np.zeros(0), np.zeros(0), len(rows)
  else:
    nmoved = 0
  n = Ji.shape[0]
  assert n <= cr.MAX_ROWS + 2, f"{n} one-sided rows: too many to enumerate"
  Minv = np.linalg.inv(M)
  found = []
  for bits in itertools.product((False, True), repeat=n):
    S = np.array(bits, bool)
    Js = np.vstack([Je, Ji[S]])
    Ds = np.concatenate([De, Di[S]])
    ars = np.concatenate([arefe, arefi[S]])
    if Js.shape[0]:
      try:
        f = np.linalg.solve(Js @ Minv @ Js.T + np.diag(1.0 / Ds), ars - Js @ a0)
      except np.linalg.LinAlgError:
        continue
    else:
      f = np.zeros(0)
    x = a0 + Minv @ (Js.T @ f)
    res = Ji @ x - arefi
    res[S] = -f[Je.shape[0]:] / Di[S]
    if np.array_equal(res < 0.0, S):
      found.append((x, f, S))
  assert len(found) == 1, f"{len(found)} consistent active sets of {n} one-sided rows"
  x, f, S = found[0]
  fi = np.zeros(n)
  fi[S] = f[Je.shape[0]:]
  Jall = np.vstack([Je, Ji])
  fall = np.concatenate([f[:Je.shape[0]], fi])
  kkt = float(np.abs(M @ (x - a0) - Jall.T @ fall).max()) if nv else 0.0
  return dict(qacc=x, f_eq=f[:Je.shape[0]], f_ineq=fi[nmoved:], f_moved=fi[:nmoved], active=S[nmoved:],
              qfrc_constraint=Jall.T @ fall, kkt=kkt)


def error_scale(M, qfrc_smooth, x, J, D, aref, always) -> np.ndarray:
  """Per-dof fp32 error scale of the Newton solution, as oracle_lib.qacc_error_scale forms it
  for problems without equalities: |H^-1| times the magnitudes of the gradient's terms at the
  solution x, H = M + sum_active J' D J.  `always`: per row, True for an equality row (active
  whatever its residual's sign)."""
  M, x = np.asarray(M, float), np.asarray(x, float)
  nv = x.size
  J = np.asarray(J, float).reshape(-1, nv)
  a = np.abs(np.asarray(qfrc_smooth, float)) + np.abs(M * x[None, :]).sum(axis=1)
  H = M.copy()
  for r in range(J.shape[0]):
    v = float(J[r] @ x - aref[r])
    if v >= 0 and not always[r]:
      continue
    a += np.abs(J[r] * D[r] * v)
    H += np.outer(J[r], J[r]) * D[r]
  return np.abs(np.linalg.inv(H)) @ a


def slide_pair_closed_form(m1, m2, arm1, arm2, gz, row) -> np.ndarray:
  """qacc of two slides along z under gravity gz coupled by one equality row (J, D, aref of
  equality_row): M = diag(m1 + arm1, m2 + arm2), a0_k = m_k gz / M_k, and for one always-active
  row x = a0 + M^-1 J' f with f = (aref - J a0) / (J M^-1 J' + 1 / D)."""
  Md = np.array([m1 + arm1, m2 + arm2])
  a0 = np.array([m1, m2]) * gz / Md
  J = row["J"][:2]
  f = (row["aref"] - J @ a0) / (J @ (J / Md) + 1.0 / row["D"])
  return a0 + J * f / Md
