"""Every narrowphase pair of the oracle against independent exact geometry (narrowphase_ref).

One small scene per pair: two free bodies with one geom each (sphere-sphere, sphere-capsule,
sphere-box, capsule-box, box-box at three size ratios), a sphere / capsule / box probe over
the plane, over a static axis-aligned box (a terrain BoxSpec), over a static box turned about
a skew axis (a jointless MJCF body, with the static geom index below and above the probe's),
and a sphere / capsule over a 9x9 heightfield.  Static scenes hold a second copy of the
static geom at (80, -60, 0), the distance of the terrain patches.  Each scene has 64 worlds:
32 poses (deterministic edge cases first, then seeded random ones), then the same poses
translated by (80, -60, 0).

Per world and pair the oracle's contacts are checked with narrowphase_ref's statements (a)
(every contact: unit normal, dist <= margin, surface points on both geoms, normal from geom 1
to geom 2) and (b) (deepest contact: the exact distance, or a translation that brings the
shapes to touch).  Tolerance 1e-9; 1e-8 where the reference's golden-section search is
involved; 1e-5 for a point inside a box.  A pose is left out of a comparison only inside a
documented band (margin +- 5e-5, kBoxFaceTie, kBoxMidEps) or, for
the direction, where the closest-point pair is not unique; never a deterministic pose, at
most 10 % of a scene's random poses, and at least half of them make a contact.

Properties of this build (MuJoCo's conventions or the build's own)
that the checks state as they are instead of as exact geometry:
  - a capsule's contacts are sphere contacts at points of its segment: the surface point of
    a contact that is not the pair's deepest may lie inside the capsule (never outside);
  - capsule-hfield uses the two segment ends (as plane-capsule), so its exact distance here
    is that of the nearer end sphere;
  - separated boxes report the largest of the 15 axis gaps: the exact distance where the
    closest features are face-vertex or edge-edge (the closest direction is one of the
    axes), a lower bound of it otherwise (vertex-vertex, vertex-edge), where the clip may
    also leave no contact;
  - a sphere centre on a capsule's axis or on another sphere's centre has normal (1, 0, 0);
  - hfield: a sphere centre below a triangle's plane (`sd < 0`) takes that plane's normal
    and depth, the build's own rule: compared with the oracle only (GPU file), never with
    the exact geometry;
  - plane-box: corners below the box centre only; exactly four of a box's corners are
    (antipodal symmetry), so the `cnt < 4` cap binds only on exact `ld == 0` ties.
"""

import dataclasses
import functools

import numpy as np
import pytest

import narrowphase_ref as R
import oracle_lib as ol
from mjlab_amd.compiler.mjcf import parse_mjcf_string
from mjlab_amd.compiler.model import BoxSpec, EntitySpec, HFieldSpec, compile_scene
from narrowphase_ref import BOX, CAPSULE, HFIELD, PLANE, SPHERE

MARGIN = 0.02
SHIFT = np.array([80.0, -60.0, 0.0])
NPOSE = 32
NCONMAX = 16

_FREE = """<body name="{n}" pos="0 0 1"><freejoint/>
  <inertial pos="0 0 0" mass="1" diaginertia="0.01 0.01 0.01"/>
  <geom name="g{n}" type="{t}" size="{s}" margin="{m}"/></body>"""
_STATIC = """<body name="{n}" pos="{p}" quat="{q}">
  <geom name="g{n}" type="box" size="{s}" margin="{m}"/></body>"""


def _fmt(v):
  return " ".join(repr(float(x)) for x in v)


def _mjcf(bodies):
  return parse_mjcf_string("<mujoco><worldbody>" + "".join(bodies) + "</worldbody></mujoco>")


def _free(name, gtype, size):
  return _FREE.format(n=name, t=gtype, s=_fmt(size), m=MARGIN)


# the static boxes: half sizes, frame; the turned one about a skew axis by 0.7 rad
ST_SIZE = np.array([0.3, 0.22, 0.15])
ST_POS = np.array([0.03, -0.02, -0.15])
ST_QUAT = R.quat_axis_angle((0.3, -0.5, 0.8), 0.7)
# the fixed body's frame of the regular scenes
FX_POS = np.array([0.01, -0.02, 0.03])
FX_QUAT = R.quat_axis_angle((0.6, 0.2, -0.4), 1.1)
IDENT = np.array([1.0, 0.0, 0.0, 0.0])


@dataclasses.dataclass
class Scene:
  name: str
  model: object
  mover: int                # free body (qpos slot) the poses move
  frame: tuple              # (pos, quat) of the fixed geom the local poses refer to
  ray: str                  # "any": random directions; "up": along the frame's +z
  gaps: tuple               # range of the random poses' gap
  q: np.ndarray = None      # (2 NPOSE, nq)
  nedge: int = 0


def _regular(name, t1, s1, t2, s2, mover, gaps=(-0.03, 0.03)):
  ent = EntitySpec("pair", _mjcf([_free("a", t1, s1), _free("b", t2, s2)]))
  m = compile_scene([ent], terrain="none", timestep=0.005)
  return Scene(name, m, mover, (FX_POS, FX_QUAT), "any", gaps)


def _plane(name, t, s):
  ent = EntitySpec("probe", _mjcf([_free("a", t, s)]))
  m = compile_scene([ent], terrain="plane", timestep=0.005)
  return Scene(name, m, 0, (np.zeros(3), IDENT), "up", (-0.03, 0.03))


def _static_aligned(name, t, s):
  ent = EntitySpec("probe", _mjcf([_free("a", t, s)]))
  boxes = [BoxSpec("terrain_0", pos=tuple(ST_POS), size=tuple(ST_SIZE)),
           BoxSpec("terrain_1", pos=tuple(ST_POS + SHIFT), size=tuple(ST_SIZE))]
  m = compile_scene([ent], terrain="generator", terrain_geoms=boxes, timestep=0.005)
  return Scene(name, m, 0, (ST_POS, IDENT), "any", (-0.03, 0.03) if t != "box" else (-0.03, 0.006))


def _static_turned(name, t, s, static_first=True):
  st = [_STATIC.format(n=f"s{k}", p=_fmt(ST_POS + k * SHIFT), q=_fmt(ST_QUAT), s=_fmt(ST_SIZE), m=0.0)
        for k in range(2)]
  probe = [_free("a", t, s)]
  ent = EntitySpec("probe", _mjcf(st + probe if static_first else probe + st))
  m = compile_scene([ent], terrain="none", timestep=0.005)
  return Scene(name, m, 0, (ST_POS, ST_QUAT), "any", (-0.03, 0.03) if t != "box" else (-0.03, 0.006))


HF_SIZE = (0.4, 0.4, 0.15, 0.05)


def _hfield(name, t, s):
  data = np.random.default_rng(5).uniform(0.0, 1.0, (9, 9))
  ent = EntitySpec("probe", _mjcf([_free("a", t, s)]))
  hfs = [HFieldSpec(f"hf{k}", pos=tuple(k * SHIFT), size=HF_SIZE, data=data) for k in range(2)]
  m = compile_scene([ent], terrain="hfield", hfields=hfs, timestep=0.005)
  return Scene(name, m, 0, (np.zeros(3), IDENT), "up", (-0.03, 0.03))


SPH, CAP = (0.06,), (0.05, 0.15)
BUILDERS = {
  "sphere_sphere": lambda n: _regular(n, "sphere", (0.06,), "sphere", (0.09,), 1),
  "sphere_capsule": lambda n: _regular(n, "sphere", SPH, "capsule", CAP, 0),
  "sphere_box": lambda n: _regular(n, "sphere", SPH, "box", (0.1, 0.1, 0.1), 0),
  "capsule_box": lambda n: _regular(n, "capsule", CAP, "box", (0.2, 0.12, 0.06), 0),
  "box_box": lambda n: _regular(n, "box", (0.1, 0.1, 0.05), "box", (0.1, 0.1, 0.06), 1, (-0.03, 0.006)),
  "box_big_small": lambda n: _regular(n, "box", (0.3, 0.25, 0.2), "box", (0.05, 0.04, 0.03), 1, (-0.02, 0.006)),
  "box_small_big": lambda n: _regular(n, "box", (0.05, 0.04, 0.03), "box", (0.3, 0.25, 0.2), 0, (-0.02, 0.006)),
  "plane_sphere": lambda n: _plane(n, "sphere", SPH),
  "plane_capsule": lambda n: _plane(n, "capsule", CAP),
  "plane_box": lambda n: _plane(n, "box", (0.12, 0.08, 0.05)),
  "static_sphere": lambda n: _static_aligned(n, "sphere", SPH),
  "static_capsule": lambda n: _static_aligned(n, "capsule", CAP),
  "static_box": lambda n: _static_aligned(n, "box", (0.12, 0.08, 0.05)),
  "turned_sphere": lambda n: _static_turned(n, "sphere", SPH),
  "turned_capsule": lambda n: _static_turned(n, "capsule", CAP),
  "turned_box_below": lambda n: _static_turned(n, "box", (0.12, 0.08, 0.05), True),
  "turned_box_above": lambda n: _static_turned(n, "box", (0.12, 0.08, 0.05), False),
  "hfield_sphere": lambda n: _hfield(n, "sphere", (0.04,)),
  "hfield_capsule": lambda n: _hfield(n, "capsule", (0.04, 0.1)),
}
SCENES = tuple(BUILDERS)


# ----------------------------------------------------------------- model -> shapes
def shapes(m, q):
  """World shapes of every geom at qpos q (free bodies and bodies welded to the world)."""
  out = []
  for g in range(m.ngeom):
    b = int(m.geom_bodyid[g])
    if b > 0 and m.body_jntnum[b] > 0:
      a = int(m.jnt_qposadr[m.body_jntadr[b]])
      bp, bq = q[a:a + 3], q[a + 3:a + 7] / np.linalg.norm(q[a + 3:a + 7])
    else:
      assert b == 0 or m.body_parentid[b] == 0
      bp, bq = np.asarray(m.body_pos[b], float), np.asarray(m.body_quat[b], float)
    Rb = R.quat_mat(bq)
    pos = bp + Rb @ np.asarray(m.geom_pos[g], float)
    rot = Rb @ R.quat_mat(m.geom_quat[g])
    kind = int(m.geom_type[g])
    tris = grid = None
    if kind == HFIELD:
      h = int(m.geom_dataid[g])
      nr, nc = int(m.hfield_nrow[h]), int(m.hfield_ncol[h])
      a = int(m.hfield_adr[h])
      data = np.asarray(m.hfield_data[a:a + nr * nc], float).reshape(nr, nc)
      tris, grid = _hf_tris(data.tobytes(), nr, nc, tuple(float(x) for x in m.hfield_size[h]))
    out.append(R.Shape(kind, np.asarray(m.geom_size[g], float), pos, rot, tris, grid))
  return out


@functools.lru_cache(maxsize=None)
def _hf_tris(raw, nr, nc, size):
  return R.hfield_triangles(np.frombuffer(raw, float).reshape(nr, nc), size)


def pairs(m, q):
  sh = shapes(m, q)
  return [(int(a), int(b), sh[a], sh[b]) for a, b in zip(m.pair_geom1, m.pair_geom2)]


def _far(A, B):
  return A.kind != PLANE and np.linalg.norm(A.pos - B.pos) > 5.0


# ----------------------------------------------------------------- poses
def _slot(sc, q, k, pos, quat):
  q[7 * k:7 * k + 3], q[7 * k + 3:7 * k + 7] = pos, quat


def _base(sc):
  """qpos with every free body but the mover at the scene's fixed frame."""
  q = np.zeros(sc.model.nq)
  for k in range(sc.model.nq // 7):
    _slot(sc, q, k, sc.frame[0], sc.frame[1])
  return q


def _local(sc, p, quat=IDENT):
  """qpos with the mover at (p, quat) given in the fixed geom's frame."""
  q = _base(sc)
  Rf = R.quat_mat(sc.frame[1])
  _slot(sc, q, sc.mover, sc.frame[0] + Rf @ np.asarray(p, float), R.quat_mul(sc.frame[1], quat))
  return q


def _gap(sc, q):
  """Exact distance of the near pair (negative: the cores meet)."""
  best = np.inf
  for _, _, A, B in pairs(sc.model, q):
    if not _far(A, B):
      c = R.closest(A, B)
      best = min(best, c.dist if (c.core > 1e-12 or A.kind == PLANE) else -1.0)
  return best


def place(sc, origin, direction, quat, gap):
  """qpos with the mover turned by `quat` (fixed frame) on the ray origin + s direction (fixed
  frame), s by bisection so that the exact distance is `gap` (gap < 0: the touching s plus
  gap).  The distance of two convex shapes grows along a ray that leaves the other's core."""
  d = np.asarray(direction, float) / np.linalg.norm(direction)
  o = np.asarray(origin, float)
  f = lambda s: _gap(sc, _local(sc, o + d * s, quat))
  lo, hi, want = 0.0, 2.0, max(gap, 0.0)
  for _ in range(44):
    mid = 0.5 * (lo + hi)
    if f(mid) > want:
      hi = mid
    else:
      lo = mid
  return _local(sc, o + d * (hi + min(gap, 0.0)), quat)


def quat_from_to(v, d):
  """Unit quaternion turning direction v onto direction d."""
  v, d = np.asarray(v, float) / np.linalg.norm(v), np.asarray(d, float) / np.linalg.norm(d)
  c = float(v @ d)
  if c < -1 + 1e-12:
    ax = np.cross(v, [1.0, 0, 0] if abs(v[0]) < 0.9 else [0, 1.0, 0])
    return R.quat_axis_angle(ax, np.pi)
  q = np.array([1.0 + c, *np.cross(v, d)])
  return q / np.linalg.norm(q)


def _far_dir(kind, size):
  """Body direction of the shape's point farthest from its centre."""
  return {SPHERE: (0, 0, 1.0), CAPSULE: (0, 0, 1.0)}.get(kind, tuple(size[:3]))


def _mover_geom(sc):
  m = sc.model
  bodies = [b for b in range(m.nbody) if m.body_jntnum[b] > 0]
  g = int(np.nonzero(np.asarray(m.geom_bodyid) == bodies[sc.mover])[0][0])
  return int(m.geom_type[g]), np.asarray(m.geom_size[g], float)


def _fixed_geom(sc):
  m = sc.model
  if m.nq == 14:
    bodies = [b for b in range(m.nbody) if m.body_jntnum[b] > 0]
    g = int(np.nonzero(np.asarray(m.geom_bodyid) == bodies[1 - sc.mover])[0][0])
  else:
    g = [g for g in range(m.ngeom) if m.body_jntnum[m.geom_bodyid[g]] == 0][0]
  return int(m.geom_type[g]), np.asarray(m.geom_size[g], float)


_QA = R.quat_axis_angle((0.2, 0.9, -0.3), 0.8)
_QX45 = R.quat_axis_angle((1, 0, 0), np.pi / 4)


def _hf_surface(sc, x, y):
  sh = [s for s in shapes(sc.model, _base(sc)) if s.kind == HFIELD][0]
  gx, gy, _ = sh.grid
  return R.hfield_height(sh.grid, float(np.clip(x, gx[0], gx[-1])), float(np.clip(y, gy[0], gy[-1])))


def edge_poses(sc):
  """The deterministic poses of a scene (fixed-frame coordinates)."""
  mk, ms = _mover_geom(sc)
  fk, fs = _fixed_geom(sc)
  up = sc.ray == "up"
  d0 = (0.0, 0.0, 1.0) if up else (0.5, -0.3, 0.8)
  o0 = (0.03, -0.02, 0.0)
  if fk == HFIELD:
    o0 = (0.03, -0.02, _hf_surface(sc, 0.03, -0.02))
  qm = _QA
  if mk == BOX and fk == BOX:  # a vertex over the face: the closest direction is a face normal
    d0 = (0.0, 0.0, 1.0)
    qm = R.quat_mul(R.quat_axis_angle((1, 0.3, 0), 0.1), quat_from_to(ms[:3], (0, 0, -1)))
  out = [place(sc, o0, d0, qm, MARGIN - 1e-4), place(sc, o0, d0, qm, MARGIN + 1e-4)]
  # the far ends of the bounding spheres toward each other
  far_m = quat_from_to(_far_dir(mk, ms), -np.asarray(d0))
  if fk in (SPHERE, CAPSULE, BOX) and not up:
    # turn the ray onto the fixed shape's farthest point instead of turning the fixed shape
    dfar = np.asarray(_far_dir(fk, fs), float)
    far_m = quat_from_to(_far_dir(mk, ms), -dfar)
    out.append(place(sc, (0, 0, 0), dfar, far_m, -0.004 if (mk, fk) == (BOX, BOX) else 0.01))
  else:
    out.append(place(sc, o0, d0, far_m, 0.01))
  r = float(ms[0])
  if (mk, fk) == (SPHERE, SPHERE):
    out.append(_local(sc, (0, 0, 0)))                      # coincident centres
  elif (mk, fk) == (SPHERE, CAPSULE):
    out.append(_local(sc, (0, 0, 0.05)))                   # on the axis, inside the segment
    out.append(_local(sc, (0, 0, fs[1] + 0.1)))            # on the axis, beyond a cap
  elif mk == SPHERE and fk == BOX:
    out.append(_local(sc, (0.03, 0.02, fs[2])))            # centre on a face
    out.append(_local(sc, (fs[0], 0.01, fs[2])))           # on an edge
    out.append(_local(sc, fs[:3]))                         # on a corner
    out.append(_local(sc, (fs[0] - 0.01, 0.01, 0.0)))      # inside, near +x
    out.append(_local(sc, (0, 0, 0)))                      # inside, at the centre
    out.append(_local(sc, (fs[0] + 0.03, fs[1] + 0.02, 0.01)))  # outside an edge
  elif mk == CAPSULE and fk in (BOX, PLANE):
    sx, sy, sz = (fs[:3] if fk == BOX else (0.5, 0.5, 0.0))
    qx = quat_from_to((0, 0, 1), (1, 0, 0))
    out.append(_local(sc, (0.01, 0.02, sz + r - 0.005), qx))   # flat on the face: 2 contacts
    out.append(_local(sc, (0.0, 0.0, sz + r + ms[1] - 0.004)))  # standing on an end
    out.append(_local(sc, (0.0, 0.0, sz + r + 0.12), R.quat_axis_angle((0, 1, 0), 0.5)))  # tilted
    if fk == BOX:
      e = np.array([1.0, 0, 1.0]) / np.sqrt(2)
      out.append(_local(sc, np.array([sx, 0.01, sz]) + e * (r - 0.005), quat_from_to((0, 0, 1), (0, 1, 0))))
      dg = np.ones(3) / np.sqrt(3)
      out.append(_local(sc, np.array([sx, sy, sz]) + dg * (r - 0.005), quat_from_to((0, 0, 1), (1, -1, 0))))
      out.append(_local(sc, (0.02, 0.01, 0.012), quat_from_to((0, 0, 1), (0.5, 0.3, 0.8))))  # axis through
      out.append(_local(sc, (0.01, 0.02, sz + 0.1)))       # one end inside
      th = 0.3                                             # across the +x top edge, ends clear
      out.append(_local(sc, (sx, 0.0, sz + 0.04), R.quat_axis_angle((0, 1, 0), np.pi / 2 + th)))
  elif mk == BOX and fk == PLANE:
    out.append(_local(sc, (0.01, 0.02, ms[2] - 0.003)))    # flat: 4
    h = (ms[1] + ms[2]) / np.sqrt(2)
    out.append(_local(sc, (0, 0, h - 0.003), _QX45))       # on an edge: 2
    out.append(_local(sc, (0, 0, np.linalg.norm(ms[:3]) - 0.003), quat_from_to(ms[:3], (0, 0, -1))))
    out.append(_local(sc, (0, 0, ms[2] + 0.004), R.quat_axis_angle((1, 0.5, 0), 0.08)))  # tilted: 4 depths
  elif mk == BOX and fk == BOX:
    top = fs[2] + ms[2]
    out.append(_local(sc, (0.01, 0.02, top - 0.003)))      # face on face
    out.append(_local(sc, (0.0, 0.0, top - 0.003), R.quat_axis_angle((0, 0, 1), np.pi / 4)))
    out.append(_local(sc, (fs[0], 0.013, top - 0.003)))    # half overhanging
    qc = quat_from_to(ms[:3], (0, 0, -1))
    out.append(_local(sc, (0.02, -0.01, fs[2] + np.linalg.norm(ms[:3]) - 0.004), qc))  # vertex into face
    qe = R.quat_mul(R.quat_axis_angle((0, 0, 1), 0.4),
                    R.quat_mul(R.quat_axis_angle((0, 1, 0), 0.3), _QX45))
    he = (ms[1] + ms[2]) / np.sqrt(2)
    out.append(_local(sc, (fs[0], 0.01, fs[2] + he - 0.006), qe))   # edge across edge, skew
    out.append(_local(sc, (0.013, 0.0, fs[2] + he - 0.004), _QX45))  # edge parallel to box 1's
    dg = fs[:3] / np.linalg.norm(fs[:3])                             # the fixed box's corner into a face
    out.append(_local(sc, fs[:3] + dg * (ms[2] - 0.004), quat_from_to((0, 0, 1), dg)))
  elif fk == HFIELD:
    gx = np.linspace(-HF_SIZE[0], HF_SIZE[0], 9)
    for i, (x, y) in enumerate((
                 (gx[3] + 0.031, gx[5] + 0.062),           # a cell's interior
                 (gx[4] + 0.05, gx[2] + 0.05),             # its diagonal
                 (gx[5], gx[3] + 0.04),                    # a grid edge
                 (gx[2], gx[6]),                           # a grid vertex
                 (gx[8] + 0.01, gx[4] + 0.03),             # just past the border
                 (gx[0], gx[0]))):                         # the field's corner
      q = quat_from_to((0, 0, 1), (1, 0.4, 0.2)) if mk == CAPSULE else IDENT
      out.append(place(sc, (x, y, _hf_surface(sc, x, y)), (0, 0, 1), q, 0.005))
      if i < 3:
        out.append(place(sc, (x, y, _hf_surface(sc, x, y)), (0, 0, 1), q, -0.01))
    for x, y in ((gx[3] + 0.02, gx[3] + 0.07), (gx[6], gx[2] + 0.05)):  # centre below the surface
      out.append(_local(sc, (x, y, _hf_surface(sc, x, y) - 0.01)))
  return out


def random_pose(sc, rng):
  mk, _ = _mover_geom(sc)
  fk, fs = _fixed_geom(sc)
  u = rng.normal(size=4)
  quat = u / np.linalg.norm(u)
  gap = rng.uniform(*sc.gaps)
  if sc.ray == "up":
    x, y = rng.uniform(-0.45, 0.45, 2)
    z = _hf_surface(sc, x, y) if fk == HFIELD else 0.0
    return place(sc, (x, y, z), (0, 0, 1), quat, gap)
  d = rng.normal(size=3)
  if sc.model.nq == 14:  # both bodies free: the fixed one turns too
    sc.frame = (rng.uniform(-0.05, 0.05, 3), rng.normal(size=4))
    sc.frame = (sc.frame[0], sc.frame[1] / np.linalg.norm(sc.frame[1]))
  return place(sc, (0, 0, 0), d, quat, gap)


@functools.lru_cache(maxsize=None)
def scene(name):
  sc = BUILDERS[name](name)
  qs = edge_poses(sc)
  sc.nedge = len(qs)
  assert sc.nedge <= NPOSE // 2, (name, sc.nedge)
  rng = np.random.default_rng(sum(map(ord, name)))
  frame = sc.frame
  while len(qs) < NPOSE:
    qs.append(random_pose(sc, rng))
  sc.frame = frame
  near = np.array(qs)
  far = near.copy()
  for k in range(sc.model.nq // 7):
    far[:, 7 * k:7 * k + 3] += SHIFT
  sc.q = np.concatenate([near, far])
  return sc


# ----------------------------------------------------------------- the checks
@dataclasses.dataclass
class Tol:
  d: float = 1e-9          # dist, pos
  n: float = 1e-9          # normal
  golden: float = 1e-8     # where the reference's segment search is involved
  inside: float = 1e-5     # a point inside a box
  mid_pos: float = 0.0     # how far along the axis a capsule-box interior point may sit off
  core_eps: float = -1.0   # cores nearer than this: the normal is undefined at the inputs' precision


def _axes15(A, B):
  ax = [A.R[:, i] for i in range(3)] + [B.R[:, i] for i in range(3)]
  for i in range(3):
    for j in range(3):
      c = np.cross(A.R[:, i], B.R[:, j])
      if np.linalg.norm(c) > 1e-9:
        ax.append(c / np.linalg.norm(c))
  return ax


def box_kind(A, B, n):
  """0 / 1 / 2: the normal is a face normal of box 1, of box 2, or of neither."""
  for k, S in ((0, A), (1, B)):
    if max(abs(float(S.R[:, i] @ n)) for i in range(3)) > 1 - 1e-6:
      return k
  return 2


def check_pair(A, B, cons, margin, tol: Tol, st: dict):
  """(a) and (b) for one pair's contacts `cons` (rows g1 g2 dist pos n) in one world.  Adds
  to st: "out" (left out of an exact comparison), "con" (has a contact)."""
  ka, kb = A.kind, B.kind
  if _far(A, B):
    assert len(cons) == 0, "contact with the far copy"
    return
  c = R.closest(A, B)
  apart = c.core > 1e-12 or ka == PLANE
  td = tol.golden if (ka, kb) == (CAPSULE, BOX) else tol.d
  ti = tol.inside if ka == CAPSULE else td   # a capsule's segment point inside a box
  rB = B.radius
  # where each contact's sphere sits (capsule / sphere against hfield, plane or box)
  centre = lambda con: con[3:6] + con[6:9] * (con[2] / 2 + rB)
  below = [ka == HFIELD and R.signed_distance(A, centre(con)) <= 0 for con in cons]
  hf_below = ka == HFIELD and any(R.signed_distance(A, p) <= 0 for p in
                                  ([B.pos] if kb == SPHERE else B.segment()))
  if hf_below:
    st["below"] = True  # the build's own sd < 0 rule: compared with the oracle only
  axis_case = True
  if (ka, kb) == (BOX, BOX) and apart:
    axis_case = max(abs(float(a @ c.n)) for a in _axes15(A, B)) > 1 - 1e-9
  mid = (ka, kb) == (CAPSULE, BOX) and c.ends - c.core > td     # an interior point is nearest
  mid_band = mid and c.ends - c.core < R.BOX_MID_EPS + 1e-6
  # ---- presence
  if not hf_below:
    if not apart:
      assert len(cons) >= 1, "cores meet, no contact"
    elif c.dist > margin + 0.5 * R.MARGIN_BAND:
      if axis_case:
        assert len(cons) == 0, f"contact at exact distance {c.dist} > margin"
    elif c.dist < margin - 0.5 * R.MARGIN_BAND - (R.BOX_MID_EPS if mid_band else 0.0):
      if axis_case:
        assert len(cons) >= 1, f"no contact at exact distance {c.dist}"
    else:
      st["out"] = True
  if len(cons) == 0:
    return
  st["con"] = True
  k = int(np.argmin(cons[:, 2]))
  # ---- (a)
  coincident = ((not apart and ka == SPHERE and kb in (SPHERE, CAPSULE) and abs(c.core) < 1e-12) or
                (ka in (SPHERE, CAPSULE, HFIELD) and abs(c.core) <= tol.core_eps))
  for i, con in enumerate(cons):
    if below[i] or coincident:  # a convention, not geometry: unit normal and depth only
      assert abs(np.linalg.norm(con[6:9]) - 1) <= tol.n and con[2] <= margin + tol.d
      continue
    deepest_exact = i == k and apart and not mid_band
    s1 = ka != CAPSULE or deepest_exact
    s2 = kb != CAPSULE or (deepest_exact and ka != HFIELD)  # hfield: the ends only
    R.check_contact(A, B, con, margin, ti if not apart else td, tol.n, (s1, s2))
    if (ka, kb) == (BOX, BOX):
      np.testing.assert_allclose(con[6:9], cons[k, 6:9], atol=0, rtol=0)
    if (ka, kb) == (CAPSULE, BOX) and not apart:
      # the segment passes through the box: no translation by one contact's depth separates
      # the pair; the box moved along +n is farther from this contact's sphere centre
      sc_ = con[3:6] - con[6:9] * (con[2] / 2 + A.radius)
      assert (R.signed_distance(B.moved(con[6:9] * R.DELTA), sc_) >
              R.signed_distance(B, sc_) + 1e-3 * R.DELTA), "box moved along n comes closer"
    elif (ka, kb) == (HFIELD, CAPSULE):  # the end sphere this contact belongs to
      R.check_direction(A, R.Shape(SPHERE, B.size, centre(con), B.R), con, td)
    elif (ka, kb) != (BOX, BOX) or i == k:
      R.check_direction(A, B, con, td, float(cons[k, 2]))
  # ---- (b)
  con = cons[k]
  d, n = float(con[2]), con[6:9]
  if below[k] or hf_below:
    return
  if coincident:  # the normal (1, 0, 0) is `expectations`' to assert, where the centres coincide exactly
    assert abs(d - (c.core - A.radius - rB)) <= td
    return
  if apart:
    if mid_band:
      st["out"] = True
      assert c.dist - td <= d <= c.dist + R.BOX_MID_EPS + td, f"dist {d} vs exact {c.dist} (mid band)"
    elif not axis_case:
      st["out"] = True
      assert d <= c.dist + td, f"axis gap {d} above the exact distance {c.dist}"
    elif (ka, kb) == (BOX, BOX) and c.dist - R.BOX_FACE_TIE - td <= d < c.dist - td:
      st["out"] = True  # a face axis preferred within kBoxFaceTie
    else:
      assert abs(d - c.dist) <= td, f"dist {d} vs exact {c.dist}"
      if c.unique and ka != PLANE:
        # the code's fixed 28 golden-section steps place a capsule's interior point to
        # 2 hl 0.618^28 along the axis; the normal turns by that over the core distance
        along = 2 * A.size[1] * 0.6180339887 ** 28 + tol.mid_pos if mid else 0.0
        assert np.abs(n - c.n).max() <= tol.n + (td + along) / c.core, f"normal {n} vs {c.n}"
      if ka == PLANE:
        assert np.abs(n - A.R[:, 2]).max() <= tol.n
  elif (ka, kb) == (CAPSULE, BOX):
    lo = c.core - A.radius
    assert d >= lo - R.BOX_FACE_TIE - td, f"dist {d} deeper than exact {lo}"
    if c.ends - c.core > 2 * R.BOX_MID_EPS:
      assert abs(d - lo) <= tol.inside + td, f"dist {d} vs exact {lo}"
    else:
      assert d <= lo + R.BOX_MID_EPS + td
  else:  # box-box overlapping, sphere centre in a box: the reported translation separates exactly
    R.check_touch_after_translation(A, B, con, td)
    if ka == SPHERE:
      lo = c.core - A.radius
      assert lo - R.BOX_FACE_TIE - tol.d <= d <= lo + tol.d, f"dist {d} vs exact {lo}"
      if d < lo - tol.d:
        st["out"] = True


def check_world(m, q, contacts, tol, margin=MARGIN):
  st = dict(out=False, con=False, below=False, kinds=set())
  for g1, g2, A, B in pairs(m, q):
    cons = contacts[(contacts[:, 0] == g1) & (contacts[:, 1] == g2)] if len(contacts) else contacts
    check_pair(A, B, cons, margin, tol, st)
    if (A.kind, B.kind) == (BOX, BOX) and len(cons):
      st["kinds"].add(box_kind(A, B, cons[0, 6:9]))
      st["maxpts"] = max(st.get("maxpts", 0), len(cons))
  return st


def check_caps(sc, stats):
  """The caps on a scene's 2 x NPOSE worlds (module docstring)."""
  for half in (0, NPOSE):
    s = stats[half:half + NPOSE]
    assert not any(x["out"] for x in s[:sc.nedge]), \
      f"deterministic pose left out: {[i for i, x in enumerate(s[:sc.nedge]) if x['out']]}"
    rnd = s[sc.nedge:]
    assert sum(x["out"] for x in rnd) <= 0.1 * len(rnd), f"{sum(x['out'] for x in rnd)} random poses left out"
    assert sum(x["con"] for x in rnd) >= 0.5 * len(rnd), f"only {sum(x['con'] for x in rnd)} random poses touch"


def oracle_contacts(sc):
  if getattr(sc, "_oracle", None) is not None:
    return sc._oracle
  out = []
  for q in sc.q:
    f = ol.forward(sc.model, q, nconmax=NCONMAX, njmax=4 * NCONMAX)
    assert f["overflow"] == 0
    out.append(f["contact"].copy())
  sc._oracle = out
  return out


@pytest.mark.parametrize("name", SCENES)
def test_oracle_pair_against_exact_geometry(name):
  sc = scene(name)
  assert sc.model.npair == (1 if sc.model.nq == 14 or "plane" in name else 2)
  stats = []
  for w, (q, con) in enumerate(zip(sc.q, oracle_contacts(sc))):
    try:
      stats.append(check_world(sc.model, q, con, Tol()))
    except AssertionError as e:
      raise AssertionError(f"{name} world {w}: {e}") from e
  check_caps(sc, stats)
  expectations(sc, [len(c) for c in oracle_contacts(sc)], stats,
               [c[0, 6:9] if len(c) else None for c in oracle_contacts(sc)])


def expectations(sc, ncon, stats, normals):
  """What the deterministic poses must show (contact counts, branches reached)."""
  name, e = sc.name, 3  # the first three poses: margin - 1e-4, margin + 1e-4, far ends
  assert ncon[0] >= 1 and ncon[1] == 0 and ncon[2] >= 1, ncon[:3]
  assert ncon[NPOSE] >= 1 and ncon[NPOSE + 1] == 0 and ncon[NPOSE + 2] >= 1, ncon[NPOSE:NPOSE + 3]
  kinds = set().union(*(s["kinds"] for s in stats))
  if name in ("sphere_sphere", "sphere_capsule") and normals is not None:
    np.testing.assert_array_equal(normals[e], [1.0, 0.0, 0.0])  # coincident centres / on the axis
  if name.endswith("capsule_box") or name in ("static_capsule", "turned_capsule"):
    assert ncon[e] == 2 and ncon[e + 1] >= 1
  if name == "plane_capsule":
    assert ncon[e] == 2 and ncon[e + 1] == 1
  if name == "plane_box":
    assert ncon[e:e + 4] == [4, 2, 1, 4], ncon[e:e + 4]
  if name in ("box_box", "static_box", "turned_box_below", "turned_box_above"):
    assert ncon[e] == 4 and ncon[e + 2] == 4 and ncon[e + 3] == 1 and ncon[e + 4] == 1, ncon[e:e + 6]
    assert stats[e + 4]["kinds"] == {2}, "edge across edge did not take the edge branch"
    assert kinds == {0, 1, 2}, kinds
  if name == "box_box":
    assert ncon[e + 1] == 8, "equal squares turned 45 degrees: 8 clipped points"
  if name == "box_big_small":
    assert 0 in kinds
  if name == "box_small_big":
    assert 1 in kinds
