"""The probe scenes of the elliptic friction cone tests (test infrastructure); every model is
compiled with cone="elliptic" and tests/elliptic_ref.py computes each world in fp64.

  slider           a sphere on three world-aligned slides on a level plane, condim 3: worlds 0-15
                   slide in 16 directions around the circle (middle zone), 16-19 are stuck (bottom
                   zone), 20-23 separate inside the margin (top zone), 24-29 slide at random angles
                   and speeds, 30-31 are beyond the margin (no contact)
  slider_impratio  the same at impratio 4
  ball_tilted3/4/6 condim_scenes' free ball on the tilted plane: condim 3, 4 selected by priority
                   (spin_plane4) and 6 as the maximum (spin_plane6, impratio 4)
  two_balls        condim_scenes' two free balls in contact, condim 6, both bodies dynamic
  pad_hinge        condim_scenes' condim-6 pad on an oblique hinge (impratio 2)
  plate            one free plate with 24 condim-3 spheres on the tilted plane: 24 contacts, 72 rows
                   (impratio 2); run again from a fast carve it exceeds (the overflow re-solve)
  mixed            five single-dof bodies (M diagonal): a limited slide at its lower limit, two
                   hinges coupled by a joint equality, a condim-1 pad and an elliptic pad (condim 3
                   by priority) on oblique hinges; rows equality pair | limit | contacts

Every scene has 32 worlds, each with its own expanded geom_friction (three distinct components),
geom_solref, geom_solimp and geom_margin and its own seeded state; the condim_scenes scenes keep
that module's fields and states.  Every dist stays at least TIE_CLEARANCE = 2e-4 >= 1e-4 from the
margin (no gaps: margin = includemargin), so the reference alone never ties (test_elliptic.py).
"""

from __future__ import annotations

import functools

import numpy as np

import condim_scenes as cds
import constraint_scenes as cs
from constraint_scenes import GRAVITY, H, NWORLD, TIE_CLEARANCE, _fmt
from mjlab_amd.spec import Spec

FIELDS = cds.FIELDS
PUCK = dict(mass=1.5, radius=0.05)
# name: (condim_scenes base or None, condim override of the ball, impratio)
TABLE = {"slider": (None, None, 1.0), "slider_impratio": (None, None, 4.0),
         "ball_tilted3": ("spin_plane4", 3, 1.0), "ball_tilted4": ("spin_plane4", None, 1.0),
         "ball_tilted6": ("spin_plane6", None, 4.0), "two_balls": ("two_balls6", None, 1.0),
         "pad_hinge": ("hinge_pad6", None, 2.0)}
SCENES = tuple(TABLE)
DIM = dict(slider=3, slider_impratio=3, ball_tilted3=3, ball_tilted4=4, ball_tilted6=6, two_balls=6, pad_hinge=6)
ROLLOUT_STEPS = 200
ROLLOUT_FRICTION = 0.6
ROLLOUT_SPEED = 1.0
ROLLOUT_ANGLE = np.deg2rad(30.0)


def impratio(name):
  return TABLE[name][2]


def scene_xml(name: str) -> str:
  base, condim, _ = TABLE[name]
  if base is not None:
    return cds.scene_xml(base, condim)
  return ('<mujoco><compiler angle="radian"/><worldbody>'
          '<geom name="floor" type="plane" size="5 5 0.1" condim="3"/>'
          '<body name="puck" pos="0 0 0"><joint name="sx" type="slide" axis="1 0 0"/>'
          '<joint name="sy" type="slide" axis="0 1 0"/><joint name="sz" type="slide" axis="0 0 1"/>'
          f'<geom name="puck" type="sphere" size="{PUCK["radius"]}" mass="{PUCK["mass"]}" condim="3"/></body>'
          '</worldbody></mujoco>')


def compile_xml(xml: str, impratio: float = 1.0, cone: str = "elliptic", **opt):
  spec = Spec.from_string(xml)
  spec.option.update(timestep=H, iterations=50, ls_iterations=50, tolerance=1e-10, impratio=impratio, cone=cone)
  spec.option.update(opt)
  return spec.compile()


@functools.lru_cache(maxsize=None)
def model(name: str):
  if name == "rollout":
    xml = scene_xml("slider").replace('condim="3"', f'condim="3" friction="{ROLLOUT_FRICTION} 0.005 0.0001"')
    return compile_xml(xml, 1.0)
  return compile_xml(scene_xml(name), impratio(name))


@functools.lru_cache(maxsize=None)
def fields(name: str) -> dict:
  base = TABLE[name][0]
  if base is not None:
    return cds.fields(base)
  m = model(name)
  rng = np.random.default_rng(2600)  # (both sliders: the same worlds, impratio apart)
  out = {f: np.tile(np.asarray(m.arrays[f], float), (NWORLD,) + (1,) * np.asarray(m.arrays[f]).ndim) for f in FIELDS}
  for w in range(NWORLD):
    for g in range(m.ngeom):
      out["geom_friction"][w, g] = [rng.uniform(0.2, 1.4), rng.uniform(0.02, 0.3), rng.uniform(0.004, 0.1)]
      out["geom_solref"][w, g] = cs._solref(rng, ((0, 0), (0, 1), (2, 0), (0, 2), (2, 2), (1, 1), (0, 0), (1, 0))[w % 8][g % 2])
      out["geom_solimp"][w, g] = cs._solimp(rng, w + 5 * (g % 2))
      out["geom_margin"][w, g] = rng.uniform(0.004, 0.03)
  return out


def slider_direction(w: int) -> float:
  """The sliding direction's angle from the x axis (worlds 0 - 15: around the circle)."""
  return 2.0 * np.pi * w / 16.0


@functools.lru_cache(maxsize=None)
def states(name: str):
  base = TABLE[name][0]
  if base is not None:
    return cds.states(base)
  f = fields(name)
  rng = np.random.default_rng(2700)
  q, qv = np.zeros((NWORLD, 3)), np.zeros((NWORLD, 3))
  c = 2 * TIE_CLEARANCE
  for w in range(NWORLD):
    margin = f["geom_margin"][w].max()
    q[w, :2] = rng.uniform(-0.5, 0.5, 2)
    if w < 16:
      dist, ang, speed, vz = -rng.uniform(c, 0.004), slider_direction(w), rng.uniform(0.5, 2.0), rng.normal(0.0, 0.05)
    elif w < 20:
      dist, ang, speed, vz = -rng.uniform(c, 0.004), rng.uniform(0, 2 * np.pi), rng.uniform(1e-4, 1e-3), 0.0
    elif w < 24:
      dist, ang, speed, vz = rng.uniform(c, margin - c), rng.uniform(0, 2 * np.pi), rng.uniform(0.1, 1.0), rng.uniform(1.0, 2.0)
    elif w < 30:
      dist = (-rng.uniform(c, 0.01), rng.uniform(c, margin - c))[w % 2]
      ang, speed, vz = rng.uniform(0, 2 * np.pi), rng.uniform(0.01, 3.0), rng.normal(0.0, 0.3)
    else:
      dist, ang, speed, vz = margin + rng.uniform(c, 0.01), rng.uniform(0, 2 * np.pi), 1.0, 0.0
    q[w, 2] = PUCK["radius"] + dist
    qv[w] = speed * np.cos(ang), speed * np.sin(ang), vz
  return q, qv


def geom_params(name: str, w: int, gname: str) -> dict:
  base, condim, _ = TABLE[name]
  if base is not None:
    p = cds.geom_params(base, w, gname)
    if condim is not None and gname == "ball":
      p["condim"] = condim
    return p
  m = model(name)
  g = int(m.names["geom"].index(gname))
  f = fields(name)
  return dict(priority=0, condim=3, friction=f["geom_friction"][w, g], solmix=float(m.arrays["geom_solmix"][g]),
              solref=f["geom_solref"][w, g], solimp=f["geom_solimp"][w, g], margin=f["geom_margin"][w, g], gap=0.0)


def world_geometry(name: str, w: int, q, qv):
  import elliptic_ref as ref
  base = TABLE[name][0]
  if base is not None:
    return cds.world_geometry(base, w, q, qv)
  b = ref.slide3_body(PUCK["mass"], q)
  n = np.array([0.0, 0.0, 1.0])
  dist = float(q[2]) - PUCK["radius"]
  return [b], "floor", "puck", None, b, dist, b.c - n * (PUCK["radius"] + 0.5 * dist), n


def reference(name: str, w: int, frame=None, mutate=None, q=None, qv=None, params=None) -> dict:
  """elliptic_ref's solution of world `w` (forward and one step) from its seeded or a given state.
  `params`: (g1, g2) geom dicts instead of the world's fields."""
  import condim_ref
  import elliptic_ref as ref
  if q is None:
    q, qv = (x[w] for x in states(name))
  bodies, g1, g2, b1, b2, dist, pos, n = world_geometry(name, w, q, qv)
  if frame is None:
    frame = cds.any_frame(n)
  p1, p2 = params if params is not None else (geom_params(name, w, g1), geom_params(name, w, g2))
  r = ref.contact_world(H, impratio(name), GRAVITY, bodies, qv, p1, p2, b1, b2, dist, pos, n, frame=frame, mutate=mutate)
  r["frame"] = np.asarray(frame, float).reshape(3, 3)
  if TABLE[name][0] is None or name == "pad_hinge":
    vn = qv + H * r["qacc"]
    r.update(qvel=vn, qpos=q + H * vn)
  else:
    qs, vs = zip(*(condim_ref.integrate_free(q[7 * k:7 * k + 7], qv[6 * k:6 * k + 6], r["qacc"][6 * k:6 * k + 6], H)
                   for k in range(len(bodies))))
    r.update(qpos=np.concatenate(qs), qvel=np.concatenate(vs))
  return r


# ----------------------------------------------------------------------------- the rollout
def rollout_params():
  A = model("rollout").arrays  # (the compiled defaults; both geoms alike)
  return tuple(dict(priority=0, condim=3, friction=np.asarray(A["geom_friction"][g], float),
                    solmix=float(A["geom_solmix"][g]), solref=np.asarray(A["geom_solref"][g], float),
                    solimp=np.asarray(A["geom_solimp"][g], float), margin=float(A["geom_margin"][g]),
                    gap=float(A["geom_gap"][g])) for g in (0, 1))


@functools.lru_cache(maxsize=None)
def rollout_start():
  """The puck at rest at its equilibrium depth (the reference settled for 300 steps), then given
  ROLLOUT_SPEED in a direction ROLLOUT_ANGLE off the frame's first tangent."""
  q, qv = np.array([0.0, 0.0, PUCK["radius"] - 1e-4]), np.zeros(3)
  for _ in range(300):
    r = reference("slider", 0, q=q, qv=qv, params=rollout_params())
    q, qv = r["qpos"], r["qvel"]
  F = cds.any_frame(np.array([0.0, 0.0, 1.0])).reshape(3, 3)
  d = np.cos(ROLLOUT_ANGLE) * F[1] + np.sin(ROLLOUT_ANGLE) * F[2]
  return q, np.array([ROLLOUT_SPEED * d[0], ROLLOUT_SPEED * d[1], 0.0]), d


@functools.lru_cache(maxsize=None)
def rollout_reference():
  """The reference's own rollout from float32 copies of the start: (qpos, qvel, max|qacc|) per step."""
  q, qv, _ = rollout_start()
  q, qv = (np.asarray(x, np.float32).astype(float) for x in (q, qv))
  qs, vs, am = [], [], []
  for _ in range(ROLLOUT_STEPS):
    r = reference("slider", 0, q=q, qv=qv, params=rollout_params())
    q, qv = r["qpos"], r["qvel"]
    qs.append(q); vs.append(qv); am.append(float(np.abs(r["qacc"]).max()))
  return np.array(qs), np.array(vs), np.array(am)


# ----------------------------------------------------------------------------- plate
# One free plate carrying 24 condim-3 spheres on the tilted plane: 24 contacts, 72 rows in one
# world -- past one row per lane and, re-solved at max capacity, the multi-round contact loops.
PLATE = dict(mass=1.0, inertia=(0.01, 0.02, 0.025), radius=0.01, nx=6, ny=4, pitch=0.04)
PLATE_NCON = PLATE["nx"] * PLATE["ny"]


def plate_spheres():
  rng = np.random.default_rng(78)
  P = PLATE
  return np.array([[(i - (P["nx"] - 1) / 2) * P["pitch"], (j - (P["ny"] - 1) / 2) * P["pitch"],
                    rng.uniform(-2e-4, 2e-4)] for j in range(P["ny"]) for i in range(P["nx"])])


@functools.lru_cache(maxsize=None)
def plate_model():
  geoms = "".join(f'<geom name="s{k}" type="sphere" size="{PLATE["radius"]}" pos="{_fmt(p)}" condim="3"/>'
                  for k, p in enumerate(plate_spheres()))
  xml = ('<mujoco><compiler angle="radian"/><worldbody>' + cds._floor(0, 3) +
         f'<body name="plate" pos="0 0 0.5" quat="{_fmt(cds.PLANE_QUAT)}"><freejoint name="root"/>'
         f'<inertial pos="0 0 0" mass="{PLATE["mass"]}" diaginertia="{_fmt(PLATE["inertia"])}"/>{geoms}</body>'
         '</worldbody></mujoco>')
  return compile_xml(xml, 2.0)


PLATE_IMPRATIO = 2.0


@functools.lru_cache(maxsize=None)
def plate_fields() -> dict:
  m = plate_model()
  rng = np.random.default_rng(2800)
  out = {f: np.tile(np.asarray(m.arrays[f], float), (NWORLD,) + (1,) * np.asarray(m.arrays[f]).ndim) for f in FIELDS}
  for w in range(NWORLD):
    for g in range(m.ngeom):
      out["geom_friction"][w, g] = [rng.uniform(0.2, 1.4), rng.uniform(0.02, 0.3), rng.uniform(0.004, 0.1)]
      out["geom_solref"][w, g] = cs._solref(rng, (0, 0, 2, 0)[(w + g) % 4])
      out["geom_solimp"][w, g] = cs._solimp(rng, w + g)
      out["geom_margin"][w, g] = rng.uniform(0.004, 0.01)
  return out


@functools.lru_cache(maxsize=None)
def plate_states():
  """Every sphere penetrates: heights within 0.2 mm, the plate 1 .. 3 mm deep, sliding and spinning."""
  rng = np.random.default_rng(2900)
  n = cds.NORMAL
  t1 = cs._unit(np.cross(n, (1.0, 0.0, 0.0)))
  q, qv = np.zeros((NWORLD, 7)), np.zeros((NWORLD, 6))
  for w in range(NWORLD):
    q[w, :3] = n * (PLATE["radius"] - rng.uniform(1e-3, 3e-3)) + t1 * rng.uniform(-0.5, 0.5)
    q[w, 3:7] = cds.PLANE_QUAT
    qv[w, :3] = rng.normal(0.0, 0.3, 3) * (0.0 if w % 4 == 3 else 1.0)
    qv[w, 3:6] = rng.normal(0.0, 1.0, 3) * (0.3, 0.3, 3.0) * (0.0 if w % 4 == 3 else 1.0)
  return q, qv


def plate_reference(w: int, order, frames, mutate=None) -> dict:
  """World `w` with its contacts in the order of sphere indices `order` and their frames (the
  engine's contact order and tangents; each frame is checked)."""
  import condim_ref
  import elliptic_ref as ref
  m = plate_model()
  f = plate_fields()
  q, qv = (x[w] for x in plate_states())
  b = condim_ref.free_body(PLATE["mass"], PLATE["inertia"], q, 0, 6)
  n = cds.NORMAL
  names = m.names["geom"]

  def params(g):
    return dict(priority=0, condim=3, friction=f["geom_friction"][w, g], solmix=float(m.arrays["geom_solmix"][g]),
                solref=f["geom_solref"][w, g], solimp=f["geom_solimp"][w, g], margin=f["geom_margin"][w, g], gap=0.0)
  cons = []
  for k, F in zip(order, frames):
    c = b.c + b.R @ plate_spheres()[k]
    dist = float(n @ c) - PLATE["radius"]
    cons.append(ref.contact_group(H, PLATE_IMPRATIO, qv, params(names.index("floor")), params(names.index(f"s{k}")),
                                  None, b, dist, c - n * (PLATE["radius"] + 0.5 * dist), n, frame=F, mutate=mutate))
  r = ref.solve_world(b.mass_matrix(), b.a0(qv, GRAVITY), cons, mutate=mutate)
  qn, vn = condim_ref.integrate_free(q, qv, r["qacc"], H)
  r.update(qpos=qn, qvel=vn, contacts=cons)
  return r


# ----------------------------------------------------------------------------- mixed
# Five single-dof bodies on the world (M diagonal, analytic): a limited slide at its lower limit,
# two hinges coupled by a joint equality, a condim-1 pad and an elliptic (condim 3 by priority)
# pad on oblique hinges touching the tilted plane.  Rows: equality pair | limit | contacts.
MIXED_LIMIT = dict(range=(-0.1, 0.1), margin=0.01, solref=(0.03, 0.8), solimp=(0.8, 0.95, 0.02, 0.4, 2.0))
MIXED_EQ = dict(polycoef=(0.01, 0.8, 0.3, 0.0, 0.0), solref=(0.03, 1.0), solimp=(0.85, 0.97, 0.01, 0.5, 2.0))
MIXED_IMPRATIO = 2.0
MIXED_PAD_OFFSET = {"pad1": -0.4, "pad3": 0.4}  # along the plane's first tangent: the dist is the pad's own


def _mixed_tangent():
  return cs._unit(np.cross(cds.NORMAL, (1.0, 0.0, 0.0)))


def _mixed_anchor(pad):
  return cds._pad_anchor() + MIXED_PAD_OFFSET[pad] * _mixed_tangent()


@functools.lru_cache(maxsize=None)
def mixed_model():
  S, Hg, P, L, E = cs.SLIDE, cs.HINGE, cds.PAD, MIXED_LIMIT, MIXED_EQ
  nogeom = 'contype="0" conaffinity="0"'
  hinge = lambda nm, x: (f'<body name="{nm}" pos="{x} 0 1"><joint name="{nm}" type="hinge" axis="{_fmt(Hg["axis"])}"'
                         f' armature="{Hg["armature"]}"/><geom type="sphere" size="{Hg["radius"]}" mass="{Hg["mass"]}"'
                         f' pos="{_fmt(Hg["com"])}" {nogeom}/></body>')
  pad = lambda nm, attrs: (f'<body name="{nm}" pos="{_fmt(_mixed_anchor(nm))}"><joint name="{nm}" type="hinge"'
                           f' axis="{_fmt(P["axis"])}" armature="{P["armature"]}"/><geom name="{nm}" type="sphere"'
                           f' size="{P["radius"]}" mass="{P["mass"]}" pos="{_fmt(P["com"])}" {attrs}/></body>')
  xml = ('<mujoco><compiler angle="radian"/><worldbody>' + cds._floor(0, 1)
         + f'<body name="sl" pos="3 0 1"><joint name="sl" type="slide" axis="{_fmt(S["axis"])}" limited="true"'
           f' range="{_fmt(L["range"])}" margin="{L["margin"]}" solreflimit="{_fmt(L["solref"])}"'
           f' solimplimit="{_fmt(L["solimp"])}" armature="{S["armature"]}"/><geom type="sphere" size="{S["radius"]}"'
           f' mass="{S["mass"]}" pos="{_fmt(S["com"])}" {nogeom}/></body>'
         + hinge("ea", 4) + hinge("eb", 5) + pad("pad1", 'condim="1"') + pad("pad3", 'condim="3" priority="1"')
         + '</worldbody><equality>'
           f'<joint joint1="ea" joint2="eb" polycoef="{_fmt(E["polycoef"])}" solref="{_fmt(E["solref"])}"'
           f' solimp="{_fmt(E["solimp"])}"/></equality></mujoco>')
  return compile_xml(xml, MIXED_IMPRATIO)


@functools.lru_cache(maxsize=None)
def mixed_fields() -> dict:
  m = mixed_model()
  rng = np.random.default_rng(3000)
  out = {f: np.tile(np.asarray(m.arrays[f], float), (NWORLD,) + (1,) * np.asarray(m.arrays[f]).ndim) for f in FIELDS}
  for w in range(NWORLD):
    for g in range(m.ngeom):
      out["geom_friction"][w, g] = [rng.uniform(0.2, 1.4), rng.uniform(0.02, 0.3), rng.uniform(0.004, 0.1)]
      out["geom_solref"][w, g] = cs._solref(rng, (0, 0, 2, 0)[(w + g) % 4])
      out["geom_solimp"][w, g] = cs._solimp(rng, w + g)
      out["geom_margin"][w, g] = rng.uniform(0.004, 0.03)
  return out


@functools.lru_cache(maxsize=None)
def mixed_states():
  """Dofs (slide, ea, eb, pad1, pad3).  Three worlds of four have the slide below its lower limit's
  margin; the pads' dists follow condim_scenes._dist, shifted by one world between the two."""
  m = mixed_model()
  f = mixed_fields()
  names = m.names["geom"]
  rng = np.random.default_rng(3100)
  q, qv = np.zeros((NWORLD, 5)), np.zeros((NWORLD, 5))
  c = 2 * TIE_CLEARANCE
  lo, mg = MIXED_LIMIT["range"][0], MIXED_LIMIT["margin"]
  for w in range(NWORLD):
    q[w, 0] = lo + mg + rng.uniform(c, 0.02) if w % 4 == 2 else lo + mg - rng.uniform(c, 0.03)
    q[w, 1:3] = rng.uniform(-0.3, 0.3, 2)
    for k, pad in ((3, "pad1"), (4, "pad3")):
      margin = max(f["geom_margin"][w, names.index("floor")], f["geom_margin"][w, names.index(pad)])
      q[w, k] = cds._pad_q(cds._dist(rng, w + (k - 3), margin))
    qv[w] = rng.normal(0.0, 1.0, 5) * (0.3, 2.0, 2.0, 3.0, 3.0)
  return q, qv


def mixed_reference(w: int, pads, frames, mutate=None) -> dict:
  """World `w` with its contacts in the order `pads` (names, the engine's contact order) and their
  frames.  The equality pair and the limit row are ordinary one-sided rows (elliptic_ref.ordinary)."""
  import condim_ref
  import elliptic_ref as ref
  import equality_ref
  m = mixed_model()
  f = mixed_fields()
  A = m.arrays
  names = m.names["geom"]
  q, qv = (x[w] for x in mixed_states())
  S, Hg, P = cs.SLIDE, cs.HINGE, cds.PAD
  g = np.asarray(GRAVITY, float)
  us = cs._unit(S["axis"])
  Ms = S["mass"] + S["armature"]
  hb = lambda anchor, B, qk, d: condim_ref.hinge_body(anchor, cs._unit(B["axis"]), B["mass"], 0.4 * B["mass"] * B["radius"] ** 2,
                                                      B["armature"], B["com"], float(qk), dof0=d, nv=5)
  bodies = {"ea": hb(np.array([4.0, 0, 1]), Hg, q[1], 1), "eb": hb(np.array([5.0, 0, 1]), Hg, q[2], 2),
            "pad1": hb(_mixed_anchor("pad1"), P, q[3], 3), "pad3": hb(_mixed_anchor("pad3"), P, q[4], 4)}
  Md = np.array([Ms] + [bodies[k].M for k in ("ea", "eb", "pad1", "pad3")])
  a0 = np.array([S["mass"] * float(us @ g) / Ms] + [float(bodies[k].a0(qv, g)[0]) for k in ("ea", "eb", "pad1", "pad3")])
  extra = []
  row = equality_ref.equality_row(dict(qadr1=1, dof1=1, qadr2=2, dof2=2, polycoef=MIXED_EQ["polycoef"],
                                       solref=MIXED_EQ["solref"], solimp=MIXED_EQ["solimp"]),
                                  q, np.zeros(5), qv, 1.0 / Md, H, 5)
  extra += [ref.ordinary(row["J"], row["D"], row["aref"]), ref.ordinary(-row["J"], row["D"], -row["aref"])]
  L = MIXED_LIMIT
  lower = q[0] - L["range"][0]
  nlim = 0
  if lower < L["margin"]:
    Jr = np.zeros(5)
    Jr[0] = 1.0
    D, ar = cr_make_row(lower, L["margin"], 1.0 / Ms, L["solref"], L["solimp"], H, float(Jr @ qv))
    extra.append(ref.ordinary(Jr, D, ar))
    nlim = 1
  assert L["range"][1] - q[0] > L["margin"] + 1e-3

  def params(gname, condim, prio):
    gi = names.index(gname)
    return dict(priority=prio, condim=condim, friction=f["geom_friction"][w, gi], solmix=float(A["geom_solmix"][gi]),
                solref=f["geom_solref"][w, gi], solimp=f["geom_solimp"][w, gi], margin=f["geom_margin"][w, gi], gap=0.0)
  n = cds.NORMAL
  every = {}
  for pad, (cd, pr) in (("pad1", (1, 0)), ("pad3", (3, 1))):
    b = bodies[pad]
    dist = float(n @ b.c) - P["radius"]
    every[pad] = (b, dist, b.c - n * (P["radius"] + 0.5 * dist), params(pad, cd, pr))
  order = list(pads) + [p for p in ("pad1", "pad3") if p not in pads]
  fr = dict(zip(pads, frames))
  cons = []
  for pad in order:
    b, dist, pos, pp = every[pad]
    F = np.asarray(fr.get(pad, cds.any_frame(n)), float)
    if F[:3] @ n < 0:  # the engine lists the pad as geom 1: the normal points from it to the floor
      cons.append(ref.contact_group(H, MIXED_IMPRATIO, qv, pp, params("floor", 1, 0), b, None, dist, pos, -n,
                                    frame=F, mutate=mutate))
    else:
      cons.append(ref.contact_group(H, MIXED_IMPRATIO, qv, params("floor", 1, 0), pp, None, b, dist, pos, n,
                                    frame=F, mutate=mutate))
    cons[-1]["pad"] = pad
  r = ref.solve_world(np.diag(Md), a0, cons, extra=extra, mutate=mutate)
  vn = qv + H * r["qacc"]
  r.update(qvel=vn, qpos=q + H * vn, contacts=[c for c in cons if c["ncon"]], nlim=nlim, nextra=len(extra))
  return r


def cr_make_row(*a):
  import constraint_ref
  return constraint_ref.make_row(*a)


# ----------------------------------------------------------------------------- by name
_single_model, _single_fields, _single_states = model, fields, states


def model(name: str):  # noqa: F811
  return plate_model() if name == "plate" else mixed_model() if name == "mixed" else _single_model(name)


def fields(name: str) -> dict:  # noqa: F811
  return plate_fields() if name == "plate" else mixed_fields() if name == "mixed" else _single_fields(name)


def states(name: str):  # noqa: F811
  return plate_states() if name == "plate" else mixed_states() if name == "mixed" else _single_states(name)
