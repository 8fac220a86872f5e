"""The probe scenes of the joint-equality tests (test infrastructure): the smallest models on
which each piece of an equality row can go wrong, and their fp64 references
(tests/equality_ref.py, tests/constraint_ref.py).  Every scene has NWORLD worlds, each with its
own seeded state; every activation test of a limit or a contact stays TIE_CLEARANCE from
equality, so that the fp32 engine and the fp64 references count the same rows.

  slide_pair  two slides on the world along z (point masses plus armature, gravity on), a `ref`
              on the second joint, polycoef "0.02 -1 0 0 0".  M is diagonal: qacc is closed form
              (equality_ref.slide_pair_closed_form), nothing comes from the oracle.
  quartic     two hinges on the world, all five coefficients non-zero; eq_data, eq_solref and
              eq_solimp expanded and distinct per world (`fields`), two worlds in seven with
              a negative (direct) solref, |pos| spread from zero to 1.3 widths of solimp, so the
              sigmoid's interior runs.
  lock        joint1 only with c0 = 0.3, and a second equality with active="false": nefc == 2.
  gripper     a horizontal hinge carrying two sibling slides with the ranges of the YAM fingers,
              polycoef "0 -1 0 0 0", a position actuator on the left finger only; half of the
              worlds have a finger limit active together with the equality.  M is coupled: the
              reference takes qM and qacc_smooth (hence qfrc_smooth) from the oracle
              (oracle_lib.forward), which ignores equalities; the limit rows are
              constraint_ref.make_row's.
  mixed       in one world: slide_pair, constraint_ref's limit_pair (its slide and its limited
              hinge) and its free ball on the tilted plane (condim 3): single-body trees, which
              mjx_model_create admits.  The three subsystems share no dof, so each has its exact
              reference; the engine solves them in one Newton problem, rows equality | limit |
              contact, every contact offset shifted.
  mixed_many  the zoo's many-legged body (model_zoo rows64) with slide_pair after it; more than
              a quarter of the worlds exceed 64 rows.  The legged dofs are the oracle's (as in
              test_gpu_model_zoo), the pair's the closed form.

quartic, lock and gripper use `generic_reference`, which also takes qM and qacc_smooth from the
oracle; tests/test_equality.py holds it to the closed form on slide_pair.
"""

from __future__ import annotations

import dataclasses
import functools

import numpy as np

import constraint_ref as cr
import constraint_scenes as cs
import equality_ref as er
import model_zoo as zoo
import oracle_lib as ol
from mjlab_amd.spec import Spec, create_position_actuator

NWORLD = 70
H = cs.H
TIE_CLEARANCE = cs.TIE_CLEARANCE
GRAVITY = cs.GRAVITY
SCENES = ("slide_pair", "quartic", "lock", "gripper", "mixed", "mixed_many")
EQ_FIELDS = ("eq_data", "eq_solref", "eq_solimp")
JNT_SLIDE, JNT_HINGE = 2, 3

# slide_pair: masses, armatures, the second joint's ref; the joints' own limit parameters differ
# from the equality's (the solref_from_joint mutant must show)
PAIR = dict(m1=0.5, m2=0.8, arm1=0.03, arm2=0.05, ref=0.04, polycoef=(0.02, -1.0, 0.0, 0.0, 0.0),
            solref=(0.015, 0.9), solimp=(0.85, 0.97, 0.004, 0.4, 2.0),
            jnt_solref=(0.05, 0.7), jnt_solimp=(0.8, 0.9, 0.01, 0.5, 2.0))
QUARTIC_COEF = (0.05, 0.8, -0.6, 0.9, -1.2)
HINGE_A = dict(axis=(0.3, 1.0, 0.2), mass=0.4, armature=0.02, com=(0.1, 0.03, 0.05), radius=0.05)
HINGE_B = dict(axis=(1.0, 0.2, -0.3), mass=0.6, armature=0.03, com=(0.02, 0.12, 0.04), radius=0.05)
# the YAM fingers' ranges (metres)
FINGER_L, FINGER_R, FINGER_MARGIN = (-0.00205, 0.037524), (-0.037524, 0.00205), 0.002
MIXED_LIMITS = dict(slide=dict(margin=0.01, solref=(0.03, 0.8), solimp=(0.8, 0.95, 0.02, 0.4, 2.0)),
                    hinge=dict(margin=0.03, solref=(0.02, 1.2), solimp=(0.7, 0.9, 0.05, 0.6, 3.0)))
MIXED_BALL = dict(margin=0.01, friction=0.7, solref=(0.025, 1.1), solimp=(0.8, 0.96, 0.01, 0.5, 2.0))
NLEG_DOF = 38  # model_zoo rows64


def _fmt(v):
  return " ".join(f"{float(x):.17g}" for x in v)


def _pair_xml(x: float) -> str:
  p = PAIR
  body = lambda nm, jn, xx, mass, arm, extra: (
    f'<body name="{nm}" pos="{xx} 0 1"><joint name="{jn}" type="slide" axis="0 0 1" armature="{arm}"'
    f' solreflimit="{_fmt(p["jnt_solref"])}" solimplimit="{_fmt(p["jnt_solimp"])}"{extra}/>'
    f'<geom type="sphere" size="0.03" mass="{mass}" contype="0" conaffinity="0"/></body>')
  return (body("pair_l", "pair_l", x, p["m1"], p["arm1"], "")
          + body("pair_r", "pair_r", x + 0.2, p["m2"], p["arm2"], f' ref="{p["ref"]}"'))


PAIR_EQ = (f'<joint name="pair" joint1="pair_l" joint2="pair_r" polycoef="{_fmt(PAIR["polycoef"])}"'
           f' solref="{_fmt(PAIR["solref"])}" solimp="{_fmt(PAIR["solimp"])}"/>')


def _hinge_xml(nm, x, j, extra=""):
  return (f'<body name="{nm}" pos="{x} 0 1"><joint name="{nm}" type="hinge" axis="{_fmt(j["axis"])}"'
          f' armature="{j["armature"]}"{extra}/><geom type="sphere" size="{j["radius"]}" mass="{j["mass"]}"'
          f' pos="{_fmt(j["com"])}" contype="0" conaffinity="0"/></body>')


def _mixed_many_model():
  """rows64's builder with the pair's two bodies after the legged tree."""
  b = zoo._rows64(112)
  p = PAIR
  lim = dict(solreflimit=_fmt(p["jnt_solref"]), solimplimit=_fmt(p["jnt_solimp"]))
  geom = lambda mass: dict(type="sphere", size="0.03", mass=str(mass), contype="0", conaffinity="0")
  for nm, x, mass, arm, extra in (("pair_l", 1.5, p["m1"], p["arm1"], {}),
                                  ("pair_r", 1.7, p["m2"], p["arm2"], dict(ref=str(p["ref"])))):
    b.roots.append(zoo.Body(nm, (x, 0.0, 1.0), (1.0, 0.0, 0.0, 0.0),
                            [zoo.Joint(nm, "slide", (0.0, 0.0, 1.0), dict(armature=str(arm), **lim, **extra))],
                            [geom(mass)]))
  xml = b.xml().replace("</mujoco>", f"<equality>{PAIR_EQ}</equality></mujoco>")
  spec = Spec.from_string(xml)
  spec.option.update(timestep=H, iterations=10, ls_iterations=20)
  for j in b.actuated:
    create_position_actuator(spec, j, stiffness=float(b.rng.uniform(8.0, 30.0)),
                             damping=float(b.rng.uniform(0.3, 1.5)), effort_limit=40.0,
                             armature=float(spec.joint(j).armature))
  return spec.compile()


@functools.lru_cache(maxsize=None)
def model(name: str):
  head = '<mujoco><compiler angle="radian"/><worldbody>'
  if name == "mixed_many":
    return _mixed_many_model()
  if name == "slide_pair":
    xml = f'{head}{_pair_xml(1.0)}</worldbody><equality>{PAIR_EQ}</equality></mujoco>'
  elif name == "quartic":
    xml = (f'{head}{_hinge_xml("qa", 1, HINGE_A)}{_hinge_xml("qb", 2, HINGE_B)}</worldbody><equality>'
           f'<joint name="quartic" joint1="qa" joint2="qb" polycoef="{_fmt(QUARTIC_COEF)}"/></equality></mujoco>')
  elif name == "lock":
    xml = (f'{head}{_hinge_xml("la", 1, HINGE_A)}'
           '<body name="lb" pos="2 0 1"><joint name="lb" type="slide" axis="0.2 0.1 1" armature="0.04"/>'
           '<geom type="sphere" size="0.03" mass="0.6" contype="0" conaffinity="0"/></body></worldbody>'
           '<default><equality solref="0.03 0.8"/></default><equality>'
           '<joint name="lock" joint1="la" polycoef="0.3"/>'
           '<joint name="off" joint1="lb" joint2="la" polycoef="0.1 2" active="false"/></equality></mujoco>')
  elif name == "gripper":
    finger = lambda nm, y, rng: (
      f'<body name="{nm}" pos="0.06 {y} 0"><joint name="{nm}" type="slide" axis="1 0 0" range="{_fmt(rng)}"'
      f' margin="{FINGER_MARGIN}" armature="0.002" damping="0.5"/><geom type="box" size="0.02 0.005 0.01"'
      ' mass="0.05" pos="0.02 0 0" contype="0" conaffinity="0"/></body>')
    xml = (f'{head}<body name="wrist" pos="0 0 0.5"><joint name="wrist" type="hinge" axis="0 1 0" armature="0.01"'
           ' damping="0.05"/><geom type="box" size="0.03 0.04 0.02" mass="0.3" pos="0.03 0 0" contype="0"'
           f' conaffinity="0"/>{finger("left_finger", 0.03, FINGER_L)}{finger("right_finger", -0.03, FINGER_R)}'
           '</body></worldbody><equality><joint name="fingers" joint1="left_finger" joint2="right_finger"'
           ' polycoef="0 -1 0 0 0"/></equality></mujoco>')
  elif name == "mixed":
    lim = lambda k: (f' limited="true" range="-0.1 0.1" margin="{MIXED_LIMITS[k]["margin"]}"'
                     f' solreflimit="{_fmt(MIXED_LIMITS[k]["solref"])}" solimplimit="{_fmt(MIXED_LIMITS[k]["solimp"])}"')
    s, bl, mb = cs.SLIDE, cs.BALL, MIXED_BALL
    xml = ('<mujoco><compiler angle="radian"/><worldbody>'
           f'<geom name="floor" type="plane" size="5 5 0.1" quat="{_fmt(cs.PLANE_QUAT)}" condim="3"/>'
           f'{_pair_xml(1.0)}'
           f'<body name="slide" pos="2 0 1"><joint name="slide" type="slide" axis="{_fmt(s["axis"])}"'
           f' armature="{s["armature"]}"{lim("slide")}/><geom type="sphere" size="{s["radius"]}" mass="{s["mass"]}"'
           f' pos="{_fmt(s["com"])}" contype="0" conaffinity="0"/></body>'
           f'{_hinge_xml("hinge", 3, cs.HINGE, lim("hinge"))}'
           '<body name="ball" pos="0 0 0.5"><freejoint name="root"/>'
           f'<inertial pos="0 0 0" mass="{bl["mass"]}" diaginertia="{_fmt(bl["inertia"])}"/>'
           f'<geom name="ball" type="sphere" size="{bl["radius"]}" condim="3" margin="{mb["margin"]}"'
           f' friction="{mb["friction"]} 0.005 0.0001" solref="{_fmt(mb["solref"])}" solimp="{_fmt(mb["solimp"])}"/>'
           f'</body></worldbody><equality>{PAIR_EQ}</equality></mujoco>')
  else:
    raise KeyError(name)
  spec = Spec.from_string(xml)
  spec.option.update(timestep=H, iterations=50, ls_iterations=50, tolerance=1e-10, impratio=1.0)
  if name == "gripper":
    create_position_actuator(spec, "left_finger", stiffness=60.0, damping=2.0, armature=0.002)
  return spec.compile()


# ----------------------------------------------------------------------------- per-world fields
@functools.lru_cache(maxsize=None)
def fields(name: str) -> dict:
  """{field: [NWORLD, ...] float64} of the scene's expanded fields (quartic only)."""
  if name != "quartic":
    return {}
  rng = np.random.default_rng(7100)
  data, sr, si = np.zeros((NWORLD, 1, 5)), np.zeros((NWORLD, 1, 2)), np.zeros((NWORLD, 1, 5))
  for w in range(NWORLD):
    data[w, 0] = np.array(QUARTIC_COEF) * rng.uniform(0.6, 1.4, 5)
    sr[w, 0] = [-rng.uniform(300.0, 3000.0), -rng.uniform(10.0, 80.0)] if w % 7 in (3, 6) else \
        [rng.uniform(0.01, 0.05), rng.uniform(0.5, 1.5)]
    dmin = rng.uniform(0.5, 0.9)
    si[w, 0] = [dmin, rng.uniform(dmin + 0.02, 0.99), rng.uniform(0.02, 0.3), rng.uniform(0.2, 0.8),
                (1.0, 2.0, 3.0)[w % 3]]
  return dict(eq_data=data, eq_solref=sr, eq_solimp=si)


def world_model(name: str, w: int):
  base = model(name)
  f = fields(name)
  if not f:
    return base
  arrays = dict(base.arrays)
  for k, v in f.items():
    arrays[k] = v[w].reshape(np.asarray(base.arrays[k]).shape)
  return dataclasses.replace(base, arrays=arrays)


# ----------------------------------------------------------------------------- states
def _pair_states(rng, n):
  q = np.stack([rng.uniform(-0.03, 0.03, n), PAIR["ref"] + rng.uniform(-0.03, 0.03, n)], axis=1)
  return q, rng.normal(0.0, 0.3, (n, 2))


def _clear_limit(x, lo, hi, mg, c):
  """x moved until neither limit's distance is within c of the margin."""
  for _ in range(100):
    if all(abs(d - mg) > c for d in (x - lo, hi - x)):
      return x
    x += 2.5 * c
  raise AssertionError("no clear state")


def _poly(c, d):
  return c[0] + d * (c[1] + d * (c[2] + d * (c[3] + d * c[4])))


@functools.lru_cache(maxsize=None)
def states(name: str):
  """Seeded (q [NWORLD, nq], qv [NWORLD, nv], ctrl [NWORLD, nu])."""
  m = model(name)
  n = NWORLD
  rng = np.random.default_rng(7300 + SCENES.index(name))
  q, qv, ctrl = np.zeros((n, m.nq)), np.zeros((n, m.nv)), np.zeros((n, m.nu))
  if name == "slide_pair":
    q, qv = _pair_states(rng, n)
  elif name == "quartic":
    f = fields(name)
    for w in range(n):
      d = rng.uniform(-0.6, 0.6)
      width = f["eq_solimp"][w, 0, 2]
      pos = rng.choice((-1.0, 1.0)) * width * 1.3 * (w % 10) / 9.0  # 0 .. 1.3 widths
      q[w] = pos + _poly(f["eq_data"][w, 0], d), d
    qv = rng.normal(0.0, 1.0, (n, 2))
  elif name == "lock":
    q = np.stack([rng.uniform(0.2, 0.4, n), rng.uniform(-0.05, 0.05, n)], axis=1)
    qv = rng.normal(0.0, 0.5, (n, 2))
  elif name == "gripper":
    c, mg = TIE_CLEARANCE, FINGER_MARGIN
    for w in range(n):
      kind = w % 4
      if kind == 0:    # the left finger within its upper margin, down to past the limit
        ql = FINGER_L[1] - mg + rng.uniform(2 * c, mg + 0.002)
      elif kind == 1:  # ... its lower
        ql = FINGER_L[0] + mg - rng.uniform(2 * c, mg + 0.001)
      else:
        ql = rng.uniform(0.006, 0.03)
      ql = _clear_limit(ql, *FINGER_L, mg, c)
      qr = _clear_limit(-ql + rng.uniform(-0.003, 0.003), *FINGER_R, mg, c)
      q[w] = rng.uniform(-1.0, 1.0), ql, qr
      qv[w] = rng.normal(0.0, 1.0), rng.normal(0.0, 0.05), rng.normal(0.0, 0.05)
      ctrl[w, 0] = ql + rng.uniform(-0.01, 0.01)
  elif name == "mixed":
    q[:, 0:2], qv[:, 0:2] = _pair_states(rng, n)
    nrm = cs._quat_z(cs.PLANE_QUAT)
    t1 = cs._unit(np.cross(nrm, (1.0, 0.0, 0.0)))
    t2 = np.cross(nrm, t1)
    for w in range(n):
      for k, key in enumerate(("slide", "hinge")):
        mg, c = MIXED_LIMITS[key]["margin"], TIE_CLEARANCE * (1.0 if k == 0 else 3.0)
        kind = (w + k) % 3
        x = rng.uniform(-0.1 + mg + 2 * c, 0.1 - mg - 2 * c) if kind == 0 else \
            -0.1 + mg - rng.uniform(2 * c, 2 * mg) if kind == 1 else 0.1 - mg + rng.uniform(2 * c, 2 * mg)
        q[w, 2 + k] = x
      qv[w, 2:4] = rng.normal(0.0, 1.0, 2) * (0.3, 1.0)
      margin, c = MIXED_BALL["margin"], 2 * TIE_CLEARANCE
      kind = w % 3
      dist = -rng.uniform(c, 0.03) if kind == 0 else rng.uniform(c, margin - c) if kind == 1 else \
          margin + rng.uniform(c, 0.01)
      q[w, 4:7] = nrm * (cs.BALL["radius"] + dist) + t1 * rng.uniform(-0.5, 0.5) + t2 * rng.uniform(-0.5, 0.5)
      q[w, 7:11] = cs._rand_quat(rng)
      qv[w, 4:7] = rng.normal(0.0, 0.4, 3)
      qv[w, 7:10] = rng.normal(0.0, 2.5, 3)
  elif name == "mixed_many":
    zm = zoo.ZooModel("mixed_many", m, dict(nv=m.nv, rows64=True, worlds=n), seed=7400)
    q, qv, ctrl = zm.states(n)
    q[:, -2:], qv[:, -2:] = _pair_states(rng, n)
  return q, qv, ctrl


# ----------------------------------------------------------------------------- references
def eq_dicts(m) -> list:
  """The model's active equalities in the form equality_ref.equality_row takes them."""
  a = m.arrays
  out = []
  for e in range(m.neq):
    if not int(a["eq_active0"][e]):
      continue
    j1, j2 = int(a["eq_obj1id"][e]), int(a["eq_obj2id"][e])
    d = dict(qadr1=int(a["jnt_qposadr"][j1]), dof1=int(a["jnt_dofadr"][j1]), qadr2=None, dof2=None,
             polycoef=np.asarray(a["eq_data"], float).reshape(-1, 5)[e],
             solref=np.asarray(a["eq_solref"], float).reshape(-1, 2)[e],
             solimp=np.asarray(a["eq_solimp"], float).reshape(-1, 5)[e],
             jnt_solref=np.asarray(a["jnt_solref"], float).reshape(-1, 2)[j1],
             jnt_solimp=np.asarray(a["jnt_solimp"], float).reshape(-1, 5)[j1])
    if j2 >= 0:
      d.update(qadr2=int(a["jnt_qposadr"][j2]), dof2=int(a["jnt_dofadr"][j2]))
    out.append(d)
  return out


def limit_rows(m, q, qv):
  """(J, D, aref) of the active joint-limit rows at (q, qv): lower dist q - lo with J = +1, upper
  dist hi - q with J = -1, each active below the joint's margin (constraint_ref.limit_pair's rule)."""
  a = m.arrays
  J, D, aref = [], [], []
  for j in range(m.njnt):
    if not int(a["jnt_limited"][j]) or int(a["jnt_type"][j]) not in (JNT_SLIDE, JNT_HINGE):
      continue
    qa, dof = int(a["jnt_qposadr"][j]), int(a["jnt_dofadr"][j])
    lo, hi = (float(x) for x in np.asarray(a["jnt_range"], float).reshape(-1, 2)[j])
    mg = float(a["jnt_margin"][j])
    for dist, sign in ((q[qa] - lo, 1.0), (hi - q[qa], -1.0)):
      if dist < mg:
        d, ar = cr.make_row(dist, mg, float(a["dof_invweight0"][dof]),
                            np.asarray(a["jnt_solref"], float).reshape(-1, 2)[j],
                            np.asarray(a["jnt_solimp"], float).reshape(-1, 5)[j], float(m.timestep), sign * qv[dof])
        r = np.zeros(m.nv)
        r[dof] = sign
        J.append(r); D.append(d); aref.append(ar)
  return np.array(J).reshape(-1, m.nv), np.array(D), np.array(aref)


def generic_reference(m, q, qv, ctrl, mutate=None, integrate=True) -> dict:
  """One world of a contact-free model with equalities and limits: qM and qacc_smooth from the
  oracle's forward (which ignores equalities), the rows from the rules, the exact solve, and the
  oracle's integration of that qacc (oracle_lib.step_given_qacc)."""
  fw = ol.forward(m, q, qv, None, ctrl, 0.0, nconmax=8, njmax=64)
  assert fw["ncon"] == 0, "generic_reference: a contact-free scene"
  M, a0 = fw["qM"], fw["qacc_smooth"]
  M = np.tril(M) + np.tril(M, -1).T
  fs = M @ a0
  rows = [er.equality_row(e, q, m.arrays["qpos0"], qv, m.arrays["dof_invweight0"], float(m.timestep), m.nv,
                          mutate) for e in eq_dicts(m)]
  Je = np.array([r["J"] for r in rows]).reshape(-1, m.nv)
  De, ae = np.array([r["D"] for r in rows]), np.array([r["aref"] for r in rows])
  Ji, Di, ai = limit_rows(m, q, qv)
  sol = er.solve(M, a0, Je, De, ae, Ji, Di, ai, mutate=mutate)
  out = dict(qacc=sol["qacc"], qfrc_constraint=sol["qfrc_constraint"], ncon=0, nlim=int(Ji.shape[0]),
             nefc=2 * len(rows) + int(Ji.shape[0]), kkt=sol["kkt"], M=M, qfrc_smooth=fs,
             J=np.vstack([Je, Ji]), D=np.concatenate([De, Di]), aref=np.concatenate([ae, ai]),
             always=np.array([True] * len(rows) + [False] * int(Ji.shape[0])), eq_pos=[r["pos"] for r in rows],
             eq_imp=[r["imp"] for r in rows])
  out["Jmag"] = np.abs(out["J"])
  if integrate:
    st = ol.step_given_qacc(m, q, qv, None, ctrl, 0.0, sol["qacc"], qfrc_constraint=sol["qfrc_constraint"],
                            qfrc_smooth=fs, nconmax=8, njmax=64)
    out.update(qvel=st["qvel"], qpos=st["qpos"])
  return out


def pair_reference(q, qv, mutate=None) -> dict:
  """slide_pair in closed form (no oracle): q, qv of its two dofs."""
  p = PAIR
  invw = np.array([1.0 / (p["m1"] + p["arm1"]), 1.0 / (p["m2"] + p["arm2"])])
  eq = dict(qadr1=0, dof1=0, qadr2=1, dof2=1, polycoef=p["polycoef"], solref=p["solref"], solimp=p["solimp"],
            jnt_solref=p["jnt_solref"], jnt_solimp=p["jnt_solimp"])
  row = er.equality_row(eq, q, np.array([0.0, p["ref"]]), qv, invw, H, 2, mutate)
  M = np.diag(1.0 / invw)
  a0 = np.array([p["m1"], p["m2"]]) * GRAVITY[2] * invw
  if mutate == "one_sided":
    a = er.solve(M, a0, row["J"], [row["D"]], [row["aref"]], mutate=mutate)["qacc"]
  else:
    a = er.slide_pair_closed_form(p["m1"], p["m2"], p["arm1"], p["arm2"], GRAVITY[2], row)
  f = -row["D"] * (row["J"] @ a - row["aref"])
  if mutate == "one_sided":
    f = max(f, 0.0)
  vn = qv + H * a
  return dict(qacc=a, qvel=vn, qpos=q + H * vn, qfrc_constraint=row["J"] * f, nefc=2, ncon=0, nlim=0,
              M=M, qfrc_smooth=M @ a0, J=row["J"][None], Jmag=np.abs(row["J"])[None], D=np.array([row["D"]]),
              aref=np.array([row["aref"]]), always=np.array([True]), eq_pos=[row["pos"]], eq_imp=[row["imp"]])


def _any_frame(n):
  t = np.cross(n, (0.0, 1.0, 0.0))
  t /= np.linalg.norm(t)
  return np.concatenate([n, t, np.cross(n, t)])


def _mixed_params():
  m = model("mixed")
  a = m.arrays
  jn, gn = m.names["joint"], m.names["geom"]
  joints = [dict(range=np.asarray(a["jnt_range"], float).reshape(-1, 2)[jn.index(k)],
                 margin=float(a["jnt_margin"][jn.index(k)]),
                 solref=np.asarray(a["jnt_solref"], float).reshape(-1, 2)[jn.index(k)],
                 solimp=np.asarray(a["jnt_solimp"], float).reshape(-1, 5)[jn.index(k)]) for k in ("slide", "hinge")]
  geoms = []
  for g in (gn.index("floor"), gn.index("ball")):
    geoms.append(dict(priority=int(a["geom_priority"][g]), condim=int(a["geom_condim"][g]),
                      friction=np.asarray(a["geom_friction"], float).reshape(-1, 3)[g],
                      solmix=float(a["geom_solmix"][g]), solref=np.asarray(a["geom_solref"], float).reshape(-1, 2)[g],
                      solimp=np.asarray(a["geom_solimp"], float).reshape(-1, 5)[g], margin=float(a["geom_margin"][g]),
                      gap=float(a["geom_gap"][g])))
  return joints, geoms


def _stack(parts, nv):
  """The block-diagonal rows of subsystems that share no dof: [(dof offset, reference dict)]."""
  J, Jm, D, aref, always = [], [], [], [], []
  for off, r in parts:
    for k in range(r["J"].shape[0]):
      row, mag = np.zeros(nv), np.zeros(nv)
      row[off:off + r["J"].shape[1]] = r["J"][k]
      mag[off:off + r["J"].shape[1]] = r["Jmag"][k]
      J.append(row); Jm.append(mag)
    D += list(r["D"]); aref += list(r["aref"])
    always += list(r.get("always", [False] * r["J"].shape[0]))
  return dict(J=np.array(J).reshape(-1, nv), Jmag=np.array(Jm).reshape(-1, nv), D=np.array(D), aref=np.array(aref),
              always=np.array(always, bool))


_refs = {}


def reference(name: str, w: int, frame=None, mutate=None) -> dict:
  """World `w`'s reference: qacc, qvel, qpos, qfrc_constraint, ncon, nefc, the rows (J, Jmag, D,
  aref, always) the force bounds are formed from, and per scene more.  `frame`: the contact
  frame whose tangents mixed's ball takes (constraint_ref.check_frame); None: any valid one."""
  key = (name, w, mutate)
  if frame is None and key in _refs:
    return _refs[key]
  q, qv, ctrl = (x[w] for x in states(name))
  emut = mutate if mutate in er.MUTANTS else None
  if name == "slide_pair":
    r = pair_reference(q, qv, emut)
  elif name in ("quartic", "lock", "gripper"):
    r = generic_reference(world_model(name, w), q, qv, ctrl, emut)
  elif name == "mixed":
    joints, (plane, ball) = _mixed_params()
    rp = pair_reference(q[0:2], qv[0:2], emut)
    rl = cr.limit_pair(cs.ref_scene("limit_pair"), joints, q[2:4], qv[2:4])
    n = cs._quat_z(cs.PLANE_QUAT)
    scene = dict(h=H, gravity=GRAVITY, impratio=1.0, plane_normal=n, plane_pos=np.zeros(3), **cs.BALL)
    rb = cr.ball_plane(scene, plane, ball, q[4:11], qv[4:10], frame=frame if frame is not None else _any_frame(n))
    cat = lambda k: np.concatenate([rp[k], rl[k], rb[k]])
    r = dict(qacc=cat("qacc"), qvel=cat("qvel"), qpos=cat("qpos"), qfrc_constraint=cat("qfrc_constraint"),
             ncon=rb["ncon"], nlim=rl["nefc"], nefc=2 + rl["nefc"] + rb["nefc"], contact_force=rb["contact_force"],
             mu=rb["mu"], ncrow=rb["nefc"], **_stack([(0, rp), (2, rl), (4, rb)], 10), eq_pos=rp["eq_pos"])
    r["M"] = np.zeros((10, 10))
    r["M"][0:2, 0:2], r["M"][2:4, 2:4], r["M"][4:, 4:] = rp["M"], rl["M"], rb["M"]
    r["qfrc_smooth"] = r["M"] @ np.concatenate([np.linalg.solve(rp["M"], rp["qfrc_smooth"]), rl["a0"], rb["a0"]])
  elif name == "mixed_many":
    m = model(name)
    st = ol.forward(m, q, qv, None, ctrl, 0.0, step=True, nconmax=64, njmax=256)
    assert not st["overflow"]
    rp = pair_reference(q[-2:], qv[-2:], emut)
    nl = NLEG_DOF
    assert m.nv == nl + 2
    r = dict(qacc=np.concatenate([st["qacc"][:nl], rp["qacc"]]), qvel=np.concatenate([st["qvel"][:nl], rp["qvel"]]),
             qpos=np.concatenate([st["qpos"][:nl + 1], rp["qpos"]]), ncon=st["ncon"], nefc=st["nefc"] + 2,
             pair=rp, **_stack([(nl, rp)], m.nv), eq_pos=rp["eq_pos"])
    r["qfrc_constraint"] = np.concatenate([np.zeros(nl), rp["qfrc_constraint"]])
  else:
    raise KeyError(name)
  if frame is None:
    _refs[key] = r
  return r


def qacc_scale(name: str, w: int) -> np.ndarray:
  """Per-dof fp32 error scale of world `w`'s qacc (the 1e-4 + 1024 eps32 s_i bound)."""
  r = reference(name, w)
  if name == "mixed_many":
    q, qv, ctrl = (x[w] for x in states(name))
    legs = ol.qacc_error_scale(model(name), q, qv, None, ctrl, 0.0, nconmax=64, njmax=256)[0][:NLEG_DOF]
    p = r["pair"]
    return np.concatenate([legs, er.error_scale(p["M"], p["qfrc_smooth"], p["qacc"], p["J"], p["D"], p["aref"],
                                                p["always"])])
  return er.error_scale(r["M"], r["qfrc_smooth"], r["qacc"], r["J"], r["D"], r["aref"], r["always"])


# ----------------------------------------------------------------------------- the gripper rollout
ROLLOUT_STEPS = 200


def rollout_ctrl(k: int) -> float:
  """The left finger's position target at step k: a sinusoid over the finger's range."""
  return 0.018 + 0.016 * np.sin(2.0 * np.pi * k / 50.0)


@functools.lru_cache(maxsize=None)
def rollout_reference():
  """200 steps of gripper's world 2 (fingers inside their ranges) under rollout_ctrl: per step
  the oracle's forward, the equality_ref solve, the oracle's integration.  Returns the largest
  |q_l + q_r| and the largest |qacc| met."""
  m = model("gripper")
  q, qv, _ = (x[2].copy() for x in states("gripper"))
  worst, amax = 0.0, 0.0
  for k in range(ROLLOUT_STEPS):
    r = generic_reference(m, q, qv, np.array([rollout_ctrl(k)]))
    q, qv = r["qpos"], r["qvel"]
    worst, amax = max(worst, abs(q[1] + q[2])), max(amax, float(np.abs(r["qacc"]).max()))
  return worst, amax
