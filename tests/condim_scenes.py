"""The probe scenes of the torsional / rolling friction tests (test infrastructure): the smallest
models on which the rows of condim-4 and condim-6 contacts can go wrong.  tests/condim_ref.py
computes the first four analytically in fp64; the oracle does not know condim > 3.

  spin_plane4   constraint_scenes' ball (2 kg, anisotropic inertia) on the tilted plane, condim 4
                selected by priority (the ball's: plane condim 1, priority 0);   6 rows
  spin_plane6   the same with condim 6 as the maximum of plane (3) and ball (6);  10 rows
  two_balls6    two free spheres of unequal mass and inertia in contact, both spinning: the
                body-1 sign of the rotational rows, `rot` summed over two bodies
  hinge_pad6    a sphere on a hinge arm touching the plane, the hinge axis oblique to the plane
                normal; M is 1 x 1 analytic: rotational rows through a non-free joint's cdof
  many70        one free plate carrying 70 small sphere geoms on the plane, 4 of condim 6 and 66
                of condim 1: 70 contacts, 106 rows -- the forms past 64 contacts and the overflow
                re-solve at max capacity (no reference: the wrench consistency check only)

Every scene has 32 worlds, each with its own copy of the expanded geom_friction (three distinct
components), geom_solref, geom_solimp and geom_margin and its own seeded state with spin about
the normal and both tangents.  Every activation test (dist against margin) stays at least
TIE_CLEARANCE 2e-4 from equality (constraint_scenes).  Worlds with w % 8 == 5 have torsional and
rolling coefficients below MINMU and a fast spin: the floor on every component shows there.
"""

from __future__ import annotations

import functools

import numpy as np

import constraint_scenes as cs
from constraint_scenes import GRAVITY, H, NWORLD, PLANE_QUAT, TIE_CLEARANCE, _fmt, _quat_z, _rand_quat, _unit
from mjlab_amd.spec import Spec

BALL = cs.BALL
BALL_B = dict(mass=0.7, inertia=(0.002, 0.0035, 0.003), radius=0.06)
PAD = dict(axis=(0.3, 1.0, 0.2), mass=0.4, armature=0.02, com=(0.1, 0.03, 0.05), radius=0.05)
PLATE = dict(mass=1.0, inertia=(0.01, 0.02, 0.025), radius=0.01, nx=10, ny=7, pitch=0.03)
PLATE_CONDIM6 = (0, 9, 33, 69)  # the plate's condim-6 spheres (the other 66: condim 1)
REF_SCENES = ("spin_plane4", "spin_plane6", "two_balls6", "hinge_pad6")
SCENES = REF_SCENES + ("many70",)
IMPRATIO = dict(spin_plane4=1.0, spin_plane6=4.0, two_balls6=1.0, hinge_pad6=2.0, many70=1.0)
MAX_CONDIM = dict(spin_plane4=4, spin_plane6=6, two_balls6=6, hinge_pad6=6, many70=6)
# the spin-down rollout: an isotropic ball on a level plane, spinning about the normal, with
# torsional friction (condim 4) and without (condim 3)
SPIN_BALL = dict(mass=2.0, inertia=(0.008, 0.008, 0.008), radius=0.1)
SPIN_FRICTION = (1.0, 0.05, 0.0001)
SPIN_OMEGA = 10.0
ROLLOUT_STEPS = 200
FIELDS = ("geom_friction", "geom_solref", "geom_solimp", "geom_margin")
NORMAL = _quat_z(PLANE_QUAT)


def _plate_spheres():
  """Local centres of the plate's 70 spheres: a 10 x 7 grid, heights within +/- 0.4 mm."""
  rng = np.random.default_rng(77)
  P = PLATE
  return np.array([[(i - (P["nx"] - 1) / 2) * P["pitch"], (j - (P["ny"] - 1) / 2) * P["pitch"],
                    rng.uniform(-4e-4, 4e-4)] for j in range(P["ny"]) for i in range(P["nx"])])


def _pad_anchor():
  """The hinge's anchor: the pad touches the plane (dist 0) at q = 0."""
  n, com = NORMAL, np.array(PAD["com"])
  t = _unit(np.cross(n, (1.0, 0.0, 0.0)))
  return n * (PAD["radius"] - n @ com) + 0.2 * t


def _floor(priority=0, condim=3):
  return (f'<geom name="floor" type="plane" size="5 5 0.1" quat="{_fmt(PLANE_QUAT)}" priority="{priority}"'
          f' condim="{condim}"/>')


def _free(name, b, attrs, pos="0 0 0.5"):
  return (f'<body name="{name}" pos="{pos}"><freejoint name="{name}_root"/>'
          f'<inertial pos="0 0 0" mass="{b["mass"]}" diaginertia="{_fmt(b["inertia"])}"/>'
          f'<geom name="{name}" type="sphere" size="{b["radius"]}" {attrs}/></body>')


def scene_xml(name: str, condim: int | None = None) -> str:
  if name == "spin_plane4":
    body = _floor(0, 1) + _free("ball", BALL, f'priority="1" condim="{4 if condim is None else condim}"')
  elif name == "spin_plane6":
    body = _floor(0, 3) + _free("ball", BALL, f'priority="0" condim="{6 if condim is None else condim}"')
  elif name == "two_balls6":
    body = _free("ball", BALL, 'condim="6"') + _free("ballb", BALL_B, 'condim="6"', pos="0.3 0 0.5")
  elif name == "hinge_pad6":
    body = (_floor(0, 6) + f'<body name="arm" pos="{_fmt(_pad_anchor())}"><joint name="hinge" type="hinge"'
            f' axis="{_fmt(PAD["axis"])}" armature="{PAD["armature"]}"/><geom name="pad" type="sphere"'
            f' size="{PAD["radius"]}" mass="{PAD["mass"]}" pos="{_fmt(PAD["com"])}" condim="6"/></body>')
  elif name == "many70":
    geoms = "".join(f'<geom name="s{k}" type="sphere" size="{PLATE["radius"]}" pos="{_fmt(p)}"'
                    f' condim="{6 if k in PLATE_CONDIM6 else 1}"/>' for k, p in enumerate(_plate_spheres()))
    body = (_floor(0, 1) + f'<body name="plate" pos="0 0 0.5" quat="{_fmt(PLANE_QUAT)}"><freejoint name="root"/>'
            f'<inertial pos="0 0 0" mass="{PLATE["mass"]}" diaginertia="{_fmt(PLATE["inertia"])}"/>{geoms}</body>')
  elif name in ("spin_down3", "spin_down4"):
    fr = f'friction="{_fmt(SPIN_FRICTION)}"'
    body = (f'<geom name="floor" type="plane" size="5 5 0.1" condim="1" {fr}/>'
            + _free("ball", SPIN_BALL, f'priority="1" condim="{name[-1]}" {fr}'))
  else:
    raise KeyError(name)
  return f'<mujoco><compiler angle="radian"/><worldbody>{body}</worldbody></mujoco>'


def compile_xml(xml: str, impratio: float = 1.0):
  spec = Spec.from_string(xml)
  spec.option.update(timestep=H, iterations=50, ls_iterations=50, tolerance=1e-10, impratio=impratio)
  return spec.compile()


@functools.lru_cache(maxsize=None)
def model(name: str):
  return compile_xml(scene_xml(name), IMPRATIO.get(name, 1.0))


@functools.lru_cache(maxsize=None)
def fields(name: str) -> dict:
  """{field: [NWORLD, ...] float64}: every world's copy of the scene's expanded fields."""
  m = model(name)
  rng = np.random.default_rng(1500 + SCENES.index(name))
  out = {f: np.tile(np.asarray(m.arrays[f], float), (NWORLD,) + (1,) * np.asarray(m.arrays[f]).ndim)
         for f in FIELDS}
  for w in range(NWORLD):
    for g in range(m.ngeom):
      # sliding, torsional (a length: a contact patch radius), rolling: three distinct components
      out["geom_friction"][w, g] = [rng.uniform(0.2, 1.4), rng.uniform(0.02, 0.3), rng.uniform(0.004, 0.1)]
      if w % 8 == 5:
        out["geom_friction"][w, g, 1:] = [rng.uniform(0.0, 5e-6), 0.0]
      out["geom_solref"][w, g] = cs._solref(rng, ((0, 0), (0, 1), (2, 0), (0, 2), (2, 2), (1, 1), (0, 0), (1, 0))[w % 8][g % 2])
      out["geom_solimp"][w, g] = cs._solimp(rng, w + 5 * (g % 2))
      out["geom_margin"][w, g] = rng.uniform(0.004, 0.03)
  return out


def _dist(rng, w, margin):
  """Three worlds of four active (penetrating or within the margin), one beyond the margin."""
  c = 2 * TIE_CLEARANCE
  kind = w % 4
  if kind in (0, 2):
    return -rng.uniform(c, 0.02)
  if kind == 1:
    return rng.uniform(c, margin - c)
  return margin + rng.uniform(c, 0.01)


def _spin(rng, w, frame_axes, scale=4.0):
  """A world angular velocity with components along the normal and both tangents; the
  below-MINMU worlds spin fast about the normal."""
  n, t1, t2 = frame_axes
  om = n * rng.normal(0.0, scale) + t1 * rng.normal(0.0, scale) + t2 * rng.normal(0.0, scale)
  if w % 8 == 5:
    om = om + n * 60.0
  return om


def _pad_q(target):
  """The hinge angle at which the pad is `target` from the plane (bisection on the exact dist)."""
  import condim_ref as ref
  a = _pad_anchor()
  f = lambda q: float(NORMAL @ ref.hinge_body(a, _unit(PAD["axis"]), PAD["mass"], 0, 0, PAD["com"], q).c) - PAD["radius"] - target
  lo, hi = -0.5, 0.5
  assert f(lo) * f(hi) < 0
  for _ in range(200):
    mid = 0.5 * (lo + hi)
    lo, hi = (mid, hi) if f(lo) * f(mid) > 0 else (lo, mid)
  return 0.5 * (lo + hi)


@functools.lru_cache(maxsize=None)
def states(name: str):
  """Seeded (q [NWORLD, nq], qv [NWORLD, nv])."""
  import constraint_ref as cr
  m = model(name)
  f = fields(name)
  rng = np.random.default_rng(1900 + SCENES.index(name))
  q, qv = np.zeros((NWORLD, m.nq)), np.zeros((NWORLD, m.nv))
  n = NORMAL
  t1 = _unit(np.cross(n, (1.0, 0.0, 0.0)))
  t2 = np.cross(n, t1)
  for w in range(NWORLD):
    margin = f["geom_margin"][w].max()
    if name in ("spin_plane4", "spin_plane6"):
      q[w, :3] = n * (BALL["radius"] + _dist(rng, w, margin)) + t1 * rng.uniform(-0.5, 0.5) + t2 * rng.uniform(-0.5, 0.5)
      q[w, 3:7] = _rand_quat(rng)
      qv[w, :3] = rng.normal(0.0, 0.4, 3)
      qv[w, 3:6] = cr.quat_mat(q[w, 3:7]).T @ _spin(rng, w, (n, t1, t2))
      if w % 8 == 5:
        # the floor's worlds: a slow approach high in the margin, spinning fast about the normal,
        # which is a principal axis there (no gyroscopic term): small qacc, so the torque of a
        # coefficient floored at MINMU stands out of its bound
        q[w, :3] = n * (BALL["radius"] + rng.uniform(0.6, 0.9) * margin)
        q[w, 3:7] = PLANE_QUAT
        qv[w, :3] = rng.normal(0.0, 0.02, 3)
        qv[w, 3:6] = (rng.normal(0.0, 0.05), rng.normal(0.0, 0.05), 300.0)
    elif name == "two_balls6":
      d = _unit(rng.normal(size=3))
      e1 = _unit(np.cross(d, (0.3, 0.5, 1.0)))
      q[w, :3] = rng.uniform(-0.3, 0.3, 3) + (0, 0, 1.0)
      q[w, 7:10] = q[w, :3] + d * (BALL["radius"] + BALL_B["radius"] + _dist(rng, w, margin))
      for a in (0, 7):
        q[w, a + 3:a + 7] = _rand_quat(rng)
      for a, b in ((0, 0), (6, 7)):
        qv[w, a:a + 3] = rng.normal(0.0, 0.4, 3)
        qv[w, a + 3:a + 6] = cr.quat_mat(q[w, b + 3:b + 7]).T @ _spin(rng, w + (4 if a else 0), (d, e1, np.cross(d, e1)))
    elif name == "hinge_pad6":
      q[w, 0] = _pad_q(_dist(rng, w, margin))
      qv[w, 0] = rng.normal(0.0, 3.0) + (40.0 if w % 8 == 5 else 0.0)
    else:  # many70: every sphere penetrates (heights within 0.4 mm, the plate 1 .. 3 mm deep)
      q[w, :3] = n * (PLATE["radius"] - rng.uniform(1e-3, 3e-3)) + t1 * rng.uniform(-0.5, 0.5)
      q[w, 3:7] = PLANE_QUAT
      qv[w, :3] = rng.normal(0.0, 0.2, 3)
      qv[w, 3:6] = rng.normal(0.0, 1.0, 3) * (0.3, 0.3, 3.0)
  return q, qv


def geom_params(name: str, w: int, gname: str) -> dict:
  m = model(name)
  g = int(m.names["geom"].index(gname))
  # (the rollout scenes have no per-world fields: the model's own values)
  f = fields(name) if name in SCENES else {k: np.asarray(m.arrays[k], float)[None] for k in FIELDS}
  w = w if name in SCENES else 0
  return dict(priority=int(m.arrays["geom_priority"][g]), condim=int(m.arrays["geom_condim"][g]),
              friction=f["geom_friction"][w, g], solmix=float(m.arrays["geom_solmix"][g]),
              solref=f["geom_solref"][w, g], solimp=f["geom_solimp"][w, g], margin=f["geom_margin"][w, g],
              gap=0.0)


def any_frame(n):
  t = _unit(np.cross(n, (0.0, 1.0, 0.0)))
  return np.concatenate([n, t, np.cross(n, t)])


def world_geometry(name: str, w: int, q=None, qv=None):
  """(bodies, g1, g2, b1, b2, dist, pos, normal) of world `w` at its seeded (or the given) state."""
  import condim_ref as ref
  if q is None:
    q, qv = (x[w] for x in states(name))
  if name in ("spin_plane4", "spin_plane6", "spin_down3", "spin_down4"):
    B, nrm = (BALL, NORMAL) if name.startswith("spin_plane") else (SPIN_BALL, np.array([0.0, 0.0, 1.0]))
    b = ref.free_body(B["mass"], B["inertia"], q, 0, 6)
    dist = float(nrm @ b.c) - B["radius"]
    return [b], "floor", "ball", None, b, dist, b.c - nrm * (B["radius"] + 0.5 * dist), nrm
  if name == "two_balls6":
    a = ref.free_body(BALL["mass"], BALL["inertia"], q[:7], 0, 12)
    b = ref.free_body(BALL_B["mass"], BALL_B["inertia"], q[7:], 6, 12)
    d = b.c - a.c
    dist = float(np.linalg.norm(d)) - BALL["radius"] - BALL_B["radius"]
    n = d / np.linalg.norm(d)
    return [a, b], "ball", "ballb", a, b, dist, a.c + n * (BALL["radius"] + 0.5 * dist), n
  if name == "hinge_pad6":
    b = ref.hinge_body(_pad_anchor(), _unit(PAD["axis"]), PAD["mass"], 0.4 * PAD["mass"] * PAD["radius"] ** 2,
                       PAD["armature"], PAD["com"], float(q[0]))
    dist = float(NORMAL @ b.c) - PAD["radius"]
    return [b], "floor", "pad", None, b, dist, b.c - NORMAL * (PAD["radius"] + 0.5 * dist), NORMAL
  raise KeyError(name)


def reference(name: str, w: int, frame=None, mutate=None, q=None, qv=None) -> dict:
  """condim_ref's solution of world `w` (forward and one step), from its seeded or a given state."""
  import condim_ref as ref
  if q is None:
    q, qv = (x[w] for x in states(name))
  bodies, g1, g2, b1, b2, dist, pos, n = world_geometry(name, w, q, qv)
  if frame is None:
    frame = any_frame(n)
  r = ref.contact_world(H, IMPRATIO.get(name, 1.0), GRAVITY, bodies, qv, geom_params(name, w, g1), geom_params(name, w, g2),
                        b1, b2, dist, pos, n, frame=frame, mutate=mutate)
  if name == "hinge_pad6":
    vn = qv + H * r["qacc"]
    r.update(qvel=vn, qpos=q + H * vn)
  else:
    qs, vs = zip(*(ref.integrate_free(q[7 * k:7 * k + 7], qv[6 * k:6 * k + 6], r["qacc"][6 * k:6 * k + 6], H)
                   for k in range(len(bodies))))
    r.update(qpos=np.concatenate(qs), qvel=np.concatenate(vs))
  return r


# ----------------------------------------------------------------------------- the GPU bounds
EPS32 = float(np.finfo(np.float32).eps)
FORCE_C = 32.0  # x eps32 (tests/test_gpu_constraint_params.py; the measurements: test_gpu_condim)


def force_bounds(r: dict, ab) -> dict:
  """tests/test_gpu_constraint_params.py's bounds of a world's forces, extended to the added
  rows.  Per row e_i = D_i sum_j |J_ij| ab_j + c eps32 D_i (|aref_i| + sum_j |J_ij| |a_j|), as its
  two parts (first, mag); qfrc_constraint_j: sum_i |J_ij| e_i; contact_force: normal sum_i e_i,
  tangent k mu_k (e_2k + e_2k+1); contact_torque component k - 2: mu_k (e_2k + e_2k+1)."""
  J, D = r["Jmag"], r["D"]
  first = D * (J @ ab)
  mag = D * (np.abs(r["aref"]) + J @ np.abs(r["qacc"]))
  mu = r["mu"]

  def wrench(e):
    pair = [mu[k] * (e[2 * k] + e[2 * k + 1]) if 2 * k + 1 < e.size else 0.0 for k in range(5)]
    return np.array([e.sum() if e.size else 0.0, pair[0], pair[1]]), np.array(pair[2:])
  (f1, t1), (fm, tm) = wrench(first), wrench(mag)
  return dict(qfrc=(J.T @ first if first.size else np.zeros(J.shape[1]), J.T @ mag if mag.size else np.zeros(J.shape[1])),
              force=(f1, fm), torque=(t1, tm))


# ----------------------------------------------------------------------------- the rollout
@functools.lru_cache(maxsize=None)
def spin_down_start():
  """(q, qv) of the rollout: the ball at rest at its equilibrium depth (the reference settled
  for 300 steps from a shallow contact), then given SPIN_OMEGA about the normal."""
  q = np.array([0.0, 0.0, SPIN_BALL["radius"] - 2e-4, 1.0, 0.0, 0.0, 0.0])
  qv = np.zeros(6)
  for _ in range(300):
    r = reference("spin_down3", 0, q=q, qv=qv)
    q, qv = r["qpos"], r["qvel"]
  qv = qv.copy()
  qv[:3] = 0.0
  qv[3:6] = (0.0, 0.0, SPIN_OMEGA)
  return q, qv


@functools.lru_cache(maxsize=None)
def spin_down_reference(name: str):
  """The reference's own rollout from float32 copies of the start: per step the spin about the
  normal after the step, the active set (the rows with a force) and the step's largest |qacc|."""
  q, qv = (np.asarray(x, np.float32).astype(float) for x in spin_down_start())
  om, sets, amax = [], [], []
  for _ in range(ROLLOUT_STEPS):
    r = reference(name, 0, q=q, qv=qv)
    q, qv = r["qpos"], r["qvel"]
    om.append(float((cs_quat_mat(q[3:7]) @ qv[3:6])[2]))
    sets.append(tuple((r["efc_force"] > 0).tolist()))
    amax.append(float(np.abs(r["qacc"]).max()))
  return np.array(om), sets, np.array(amax)


def cs_quat_mat(q):
  import constraint_ref as cr
  return cr.quat_mat(q)
