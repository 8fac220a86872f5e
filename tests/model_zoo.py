"""Deterministic synthetic models beyond the two robots (test infrastructure, no assets).

Every GPU test of the engine used to run a G1 (35 dofs), a Go1 (18 dofs) or a one- or two-body
toy.  The zoo generates MJCF strings for body trees the engine supports but no robot has, and
compiles them through `mjlab_amd.spec.Spec` as tests/invariants.py does:

  - one model per generic register-row length of csrc/engine.hip (`MJX_GENERIC_NRS`), at the
    smallest and the largest dof count that selects each, and every dof count mod 4 above 36;
  - `wave64`: 64 dofs on 64 bodies (a fixed base: 63 moving bodies plus the world, the first
    with two joints -- a free joint would spend six dofs on one body); `wave60` and `free57`,
    the same at the 60 dofs the engine admits and at the smallest count of that row length;
  - `chain24`: a fixed-base chain 24 levels deep of alternating hinges and slides;
  - `multitree`: two articulated free trees of 8 and 12 bodies more than 1 m apart, so that the
    level order of the bodies differs from their id order; it also holds a body with three
    joints (hinge, hinge, slide), a body with seven children and bodies with exactly five and
    six children (the engine packs the first five into its body record); `multitree_arm` adds
    a fixed-base arm beside them; `fallbacks26` has the same joint and child counts in one tree;
  - `robot_object`: an articulated free tree followed by a single free body, the last id;
  - `rows64`: a many-legged free tree whose seeded worlds make at most 64 and more than 64
    constraint rows (the engine's lane-per-row boundary), below the 160-row fast carve;
  - `params14`, `params38`: free trees (padded to 16 dofs: the lane-group form of the Jacobian
    loop; to 40: one lane per dof) whose geoms, floor and limited joints carry non-default
    constraint parameters in the MJCF: priority 0 / 1, condim 1 / 3, own friction, solmix,
    solref (some in the direct negative form), solimp, margin and gap; limit margins, solreflimit
    and solimplimit, and some ranges narrower than twice the margin.  Their states put a contact
    in its gap (margin - gap <= dist < margin) and both sides of a limit at once in at least a
    quarter of the worlds each, every activation test TIE_CLEARANCE from equality.

Every model has skewed joint axes, geoms offset from the body origin (offset inertias),
non-identity body quaternions, some armature, damping and stiffness (with a springref away
from the sampled state), some limited joints, position actuators on every third joint, a few
sensors, and sphere / capsule collision geoms against one plane only (narrowphase is tested
elsewhere).  A world stays within about 3 m of the origin.

The engine refuses the models in `REJECTED` when it creates them (more than 60 dofs; a tree after
a tree of several bodies): they are oracle-only until it can compute them.  `RUNNABLE` is the rest.

`get(name)` is a `ZooModel`: `.model` (compiled once), `.states(n)` (seeded q, qv, ctrl) and
`.props` (what it was built for).
"""

from __future__ import annotations

import copy
import functools
from dataclasses import dataclass, field

import numpy as np

from mjlab_amd.spec import Spec, create_position_actuator

GEOM_PLANE, GEOM_SPHERE, GEOM_CAPSULE = 0, 2, 3
JNT_FREE, JNT_SLIDE, JNT_HINGE = 0, 2, 3
TIE_CLEARANCE = 2e-4  # no colliding surface point this close to the plane in a sampled state


# ----------------------------------------------------------------------------- tree description
@dataclass
class Joint:
  name: str
  type: str  # "hinge" | "slide" | "free"
  axis: tuple = (0.0, 0.0, 1.0)
  attrs: dict = field(default_factory=dict)


@dataclass
class Body:
  name: str
  pos: tuple
  quat: tuple
  joints: list = field(default_factory=list)
  geoms: list = field(default_factory=list)  # XML attribute dicts
  sites: list = field(default_factory=list)
  children: list = field(default_factory=list)
  depth: int = 0


def _fmt(v) -> str:
  return " ".join(f"{float(x):.6g}" for x in v)


def _unit(v):
  v = np.asarray(v, float)
  return v / np.linalg.norm(v)


class Builder:
  """Seeded generator of bodies, joints and geoms; collects actuated joints and sensors."""

  floor_attrs = ""  # further XML attributes of the plane

  def __init__(self, seed: int, collide: bool = True):
    self.rng = np.random.default_rng(seed)
    self.collide = collide
    self.roots: list[Body] = []
    self.njoint = 0
    self.nbody = 0
    self.actuated: list[str] = []
    self.sensors: list[str] = []

  # -- pieces
  def quat(self, angle=0.6):
    ax = _unit(self.rng.normal(size=3))
    th = self.rng.uniform(0.15, angle)
    return (np.cos(th / 2), *(ax * np.sin(th / 2)))

  def geom(self, kind=None, collide=None, reach=0.08):
    """One sphere or capsule offset from the body origin (mass given, inertia from it)."""
    rng = self.rng
    kind = kind or ("capsule" if rng.random() < 0.5 else "sphere")
    collide = self.collide if collide is None else collide
    g = dict(type=kind, mass=f"{rng.uniform(0.15, 0.8):.4g}",
             contype="0", conaffinity="1" if collide else "0")
    off = rng.uniform(-0.03, 0.03, 3)
    if kind == "sphere":
      g.update(size=f"{rng.uniform(0.025, 0.045):.4g}", pos=_fmt(off))
    else:
      tip = off + _unit(rng.normal(size=3)) * rng.uniform(0.5, 1.0) * reach
      g.update(size=f"{rng.uniform(0.015, 0.03):.4g}", fromto=_fmt([*off, *tip]))
    return g

  def joint(self, type="hinge"):
    """A hinge or slide with a skewed axis; every third one actuated, some sprung, damped,
    limited or with armature (deterministic in the joint's index, so every model has each)."""
    rng = self.rng
    k = self.njoint
    self.njoint += 1
    name = f"j{k}"
    a = {}
    if k % 2 == 0:
      a["armature"] = f"{rng.uniform(0.005, 0.03):.4g}"
    if k % 3 != 1:
      a["damping"] = f"{rng.uniform(0.05, 0.4):.4g}"
    if k % 4 == 1:  # a spring whose reference is away from the sampled state
      a["stiffness"] = f"{rng.uniform(2.0, 12.0):.4g}"
      a["springref"] = "0.9" if type == "hinge" else "0.15"
    if k % 5 == 2:
      a["limited"] = "true"
      a["range"] = "-0.35 0.35" if type == "hinge" else "-0.05 0.05"
    if k % 3 == 0:
      self.actuated.append(name)
    if k % 7 == 3:
      self.sensors.append(f'<jointpos name="sp{k}" joint="{name}"/>')
      self.sensors.append(f'<jointvel name="sv{k}" joint="{name}"/>')
    return Joint(name, type, tuple(_unit(rng.normal(size=3))), a)

  def body(self, parent: Body | None, pos, joints, geoms=None, quat=None):
    k = self.nbody
    self.nbody += 1
    b = Body(f"b{k}", tuple(pos), tuple(quat if quat is not None else self.quat()), list(joints),
             geoms if geoms is not None else [self.geom()], depth=0 if parent is None else parent.depth + 1)
    if k % 6 == 2:
      b.sites.append(dict(name=f"s{k}", pos=_fmt(self.rng.uniform(-0.03, 0.03, 3)), quat=_fmt(self.quat())))
      self.sensors += [f'<gyro name="gy{k}" site="s{k}"/>', f'<velocimeter name="ve{k}" site="s{k}"/>',
                       f'<accelerometer name="ac{k}" site="s{k}"/>', f'<framepos name="fp{k}" site="s{k}"/>']
    (self.roots if parent is None else parent.children).append(b)
    return b

  def free_root(self, pos):
    b = self.body(None, pos, [Joint(f"free{self.nbody}", "free")], [self.geom("capsule", reach=0.15)],
                  quat=(1.0, 0.0, 0.0, 0.0))
    self.sensors.append(f'<subtreeangmom name="am{b.name}" body="{b.name}"/>')
    return b

  def grow(self, root: Body, n: int, slide_p=0.25, max_children=4, max_depth=7):
    """`n` one-joint bodies under `root`, each below a random body that still has room."""
    rng = self.rng
    pool = [root]
    for _ in range(n):
      room = [b for b in pool if len(b.children) < max_children and b.depth - root.depth < max_depth]
      p = room[int(rng.integers(len(room)))]
      d = _unit(rng.normal(size=3) + np.array([0.0, 0.0, -0.6]))
      c = self.body(p, d * rng.uniform(0.06, 0.12),
                    [self.joint("slide" if rng.random() < slide_p else "hinge")])
      pool.append(c)
    return pool

  # -- XML
  def _body_xml(self, b: Body, ind: str) -> list[str]:
    out = [f'{ind}<body name="{b.name}" pos="{_fmt(b.pos)}" quat="{_fmt(b.quat)}">']
    for j in b.joints:
      if j.type == "free":
        out.append(f'{ind}  <freejoint name="{j.name}"/>')
      else:
        extra = "".join(f' {k}="{v}"' for k, v in j.attrs.items())
        out.append(f'{ind}  <joint name="{j.name}" type="{j.type}" axis="{_fmt(j.axis)}"'
                   f' pos="{_fmt(self.rng.uniform(-0.02, 0.02, 3))}"{extra}/>')
    for g in b.geoms:
      out.append(f"{ind}  <geom" + "".join(f' {k}="{v}"' for k, v in g.items()) + "/>")
    for s in b.sites:
      out.append(f"{ind}  <site" + "".join(f' {k}="{v}"' for k, v in s.items()) + "/>")
    for c in b.children:
      out += self._body_xml(c, ind + "  ")
    out.append(f"{ind}</body>")
    return out

  def xml(self) -> str:
    lines = ['<mujoco>', '  <compiler angle="radian"/>', '  <option timestep="0.004"/>', '  <worldbody>',
             f'    <geom name="floor" type="plane" size="5 5 0.1" contype="1" conaffinity="0"{self.floor_attrs}/>']
    for r in self.roots:
      lines += self._body_xml(r, "    ")
    lines += ['  </worldbody>', '  <sensor>'] + ["    " + s for s in self.sensors] + ['  </sensor>', '</mujoco>']
    return "\n".join(lines)

  def compile(self):
    spec = Spec.from_string(self.xml())
    spec.option.update(timestep=0.004, iterations=10, ls_iterations=20)
    for j in self.actuated:
      create_position_actuator(spec, j, stiffness=float(self.rng.uniform(8.0, 30.0)),
                               damping=float(self.rng.uniform(0.3, 1.5)), effort_limit=40.0,
                               armature=float(spec.joint(j).armature))
    return spec.compile()


class ParamBuilder(Builder):
  """A Builder whose geoms, floor and limited joints have non-default constraint parameters."""

  floor_attrs = (' priority="0" condim="3" friction="0.8 0.005 0.0001" solmix="0.6" solref="0.015 0.9"'
                 ' solimp="0.85 0.97 0.004 0.4 3" margin="0.006" gap="0.003"')

  def __init__(self, seed: int):
    super().__init__(seed)
    self.ngeom = 0

  def _solimp(self):
    rng = self.rng
    dmin = rng.uniform(0.6, 0.9)
    return _fmt([dmin, rng.uniform(dmin, 0.98), rng.uniform(0.002, 0.02), rng.uniform(0.3, 0.7),
                 float(rng.integers(1, 4))])

  def geom(self, kind=None, collide=None, reach=0.08):
    g = super().geom(kind, collide, reach)
    rng, k = self.rng, self.ngeom
    self.ngeom += 1
    margin = rng.uniform(0.004, 0.02)
    solref = [-rng.uniform(500.0, 2000.0), -rng.uniform(20.0, 60.0)] if k % 4 == 1 else \
      [rng.uniform(0.012, 0.04), rng.uniform(0.7, 1.3)]
    g.update(priority=str(k % 2), condim="3" if k % 3 else "1",
             friction=_fmt([rng.uniform(0.4, 1.3), 0.005, 0.0001]), solmix=f"{rng.uniform(0.3, 2.0):.4g}",
             solref=_fmt(solref), solimp=self._solimp(), margin=f"{margin:.4g}",
             gap=f"{margin * rng.uniform(0.3, 0.7):.4g}")
    return g

  def joint(self, type="hinge"):
    j = super().joint(type)
    if "limited" in j.attrs:
      rng = self.rng
      k = int(j.name[1:])
      scale = 3.0 if type == "hinge" else 1.0  # radians, metres
      margin = scale * rng.uniform(0.006, 0.02)
      if k % 10 == 2:  # narrower than twice the margin: both limit rows can be active at once
        half = 0.5 * margin * rng.uniform(0.8, 1.4)
        j.attrs["range"] = f"{-half:.5g} {half:.5g}"
      j.attrs.update(margin=f"{margin:.5g}", solreflimit=_fmt([rng.uniform(0.01, 0.04), rng.uniform(0.7, 1.3)]),
                     solimplimit=self._solimp())
    return j


def _param_tree(nv, seed):
  b = ParamBuilder(seed)
  b.grow(b.free_root((0.0, 0.0, 0.6)), nv - 6)
  return b


# ----------------------------------------------------------------------------- the models
def _free_tree(nv, seed, pos=(0.0, 0.0, 0.6), **kw):
  b = Builder(seed)
  b.grow(b.free_root(pos), nv - 6, **kw)
  return b


def _fixed_tree(nv, seed, pos=(0.0, 0.0, 1.2), **kw):
  b = Builder(seed)
  root = b.body(None, pos, [b.joint("hinge")])
  b.grow(root, nv - 1, **kw)
  return b


def _wave64(seed):
  """64 dofs on 64 bodies: the world plus 63 moving bodies, the first with two joints."""
  b = Builder(seed)
  root = b.body(None, (0.0, 0.0, 1.4), [b.joint("hinge"), b.joint("slide")])
  b.grow(root, 62, max_children=4, max_depth=6)
  return b


def _chain24(seed):
  """A fixed-base chain of 24 bodies, hinge and slide alternating (24 levels below the world)."""
  b = Builder(seed)
  p = None
  for k in range(24):
    d = _unit(b.rng.normal(size=3) * 0.5 + np.array([1.0, 0.0, -0.2]))
    p = b.body(p, (0.0, 0.0, 1.5) if p is None else d * 0.07, [b.joint("slide" if k % 2 else "hinge")])
  return b


def _multitree(seed, arm=False):
  """Tree A (8 bodies, 15 dofs): a free hub with seven children, one of them with three joints
  (hinge, hinge, slide).  Tree B (12 bodies, 17 dofs), 1.4 m away: a free hub with exactly five
  children, one of which has exactly six.  Body ids run tree by tree, levels interleave them."""
  b = Builder(seed)
  rng = b.rng
  ring = lambda k, n, r: (r * np.cos(2 * np.pi * k / n), r * np.sin(2 * np.pi * k / n), rng.uniform(-0.08, -0.03))
  a = b.free_root((-0.7, 0.0, 0.5))
  for k in range(7):
    joints = [b.joint("hinge"), b.joint("hinge"), b.joint("slide")] if k == 3 else [b.joint("hinge")]
    b.body(a, ring(k, 7, 0.12), joints)
  r = b.free_root((0.7, 0.1, 0.5))
  five = [b.body(r, ring(k, 5, 0.12), [b.joint("slide" if k == 1 else "hinge")]) for k in range(5)]
  for k in range(6):
    b.body(five[2], ring(k, 6, 0.09), [b.joint("slide" if k == 4 else "hinge")])
  if arm:  # a fixed-base arm beside them: 5 more dofs, a third tree whose root is not free
    p = None
    for k in range(5):
      p = b.body(p, (0.0, 0.9, 0.9) if p is None else (0.1, 0.0, -0.05), [b.joint("slide" if k == 2 else "hinge")])
  return b


def _fallbacks(seed):
  """One free tree with multitree's shapes: a hub with seven children, one of them with three
  joints (hinge, hinge, slide), one with exactly five children and one with exactly six."""
  b = Builder(seed)
  rng = b.rng
  ring = lambda k, n, r: (r * np.cos(2 * np.pi * k / n), r * np.sin(2 * np.pi * k / n), rng.uniform(-0.08, -0.03))
  hub = b.free_root((0.0, 0.0, 0.6))
  arms = []
  for k in range(7):
    joints = [b.joint("hinge"), b.joint("hinge"), b.joint("slide")] if k == 3 else [b.joint("hinge")]
    arms.append(b.body(hub, ring(k, 7, 0.14), joints))
  for k in range(5):
    b.body(arms[0], ring(k, 5, 0.08), [b.joint("slide" if k == 1 else "hinge")])
  for k in range(6):
    b.body(arms[4], ring(k, 6, 0.08), [b.joint("slide" if k == 4 else "hinge")])
  return b


def _wave60(seed):
  """60 dofs on 60 bodies, the most the engine admits: the world plus 59 moving bodies, the
  first with two joints (hinge, slide)."""
  b = Builder(seed)
  root = b.body(None, (0.0, 0.0, 1.4), [b.joint("hinge"), b.joint("slide")])
  b.grow(root, 58, max_children=4, max_depth=6)
  return b


def _robot_object(seed):
  """An articulated free tree (15 dofs) and then one free sphere, whose body id is the last."""
  b = Builder(seed)
  b.grow(b.free_root((0.0, 0.0, 0.6)), 9)
  b.free_root((0.5, 0.3, 0.3)).geoms[:] = [b.geom("sphere")]
  return b


def _rows64(seed):
  """A free trunk with sixteen two-hinge legs whose feet (twelve spheres, four flat capsules)
  end at one height, and four spheres under the trunk: up to 24 contacts, 96 contact rows."""
  b = Builder(seed, collide=False)
  rng = b.rng
  trunk = b.free_root((0.0, 0.0, 0.4))
  trunk.geoms[:] = [dict(type="capsule", fromto="-0.5 0 0 0.5 0 0", size="0.04", mass="3.0",
                         contype="0", conaffinity="0")]
  trunk.geoms += [dict(type="sphere", pos=_fmt((x, 0.0, -0.31)), size="0.03", mass="0.1", contype="0",
                       conaffinity="1") for x in (-0.4, -0.15, 0.15, 0.4)]
  for k in range(16):
    x, side = -0.45 + 0.12 * (k // 2), 1.0 if k % 2 else -1.0
    thigh = b.body(trunk, (x, 0.1 * side, -0.02), [b.joint("hinge")],
                   [dict(type="capsule", fromto=_fmt((0, 0, 0, 0.02, 0.05 * side, -0.15)), size="0.02",
                         mass=f"{rng.uniform(0.2, 0.5):.4g}", contype="0", conaffinity="0")],
                   quat=(1.0, 0.0, 0.0, 0.0))
    if k % 4 == 3:
      foot = dict(type="capsule", fromto=_fmt((-0.04, 0, -0.15, 0.04, 0, -0.15)), size="0.03")
    else:
      foot = dict(type="sphere", pos="0 0 -0.15", size="0.03")
    foot.update(mass=f"{rng.uniform(0.1, 0.3):.4g}", contype="0", conaffinity="1")
    yaw = 0.25 * side * (1 + k % 3)  # shins turned about the vertical: the feet stay level
    b.body(thigh, (0.02, 0.05 * side, -0.15), [b.joint("hinge")], [foot],
           quat=(np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)))
  return b


# name -> (factory, properties the model was built for).  nv is asserted by the CPU tests.
_RECIPES = {
  "free7": (lambda: _free_tree(7, 101), dict(nv=7)),
  "free12": (lambda: _free_tree(12, 102), dict(nv=12)),
  "slide13": (lambda: _fixed_tree(13, 103, slide_p=0.7), dict(nv=13, slide_heavy=True, fixed=True)),
  "free16": (lambda: _free_tree(16, 104), dict(nv=16)),
  "free18": (lambda: _free_tree(18, 105), dict(nv=18)),
  "robot_object": (lambda: _robot_object(106), dict(nv=21, robot_object=True, trees=2)),
  "chain24": (lambda: _chain24(107), dict(nv=24, chain=True, fixed=True, levels=25)),
  "free29": (lambda: _free_tree(29, 108), dict(nv=29)),
  "multitree": (lambda: _multitree(109), dict(nv=32, multitree=True, trees=2, max_children=7,
                                              max_joints=3, child_counts=(5, 6, 7))),
  "free35": (lambda: _free_tree(35, 110), dict(nv=35)),
  "multitree_arm": (lambda: _multitree(111, arm=True), dict(nv=37, multitree=True, trees=3, max_children=7,
                                                            max_joints=3, child_counts=(5, 6, 7))),
  "rows64": (lambda: _rows64(112), dict(nv=38, rows64=True, worlds=32)),
  "fixed39": (lambda: _fixed_tree(39, 113), dict(nv=39, fixed=True)),
  "free40": (lambda: _free_tree(40, 114), dict(nv=40)),
  "free45": (lambda: _free_tree(45, 115), dict(nv=45)),
  "star48": (lambda: _fixed_tree(48, 116, max_children=8, max_depth=3), dict(nv=48, fixed=True, star=True)),
  "free53": (lambda: _free_tree(53, 117), dict(nv=53)),
  "fixed56": (lambda: _fixed_tree(56, 118), dict(nv=56, fixed=True)),
  "free61": (lambda: _free_tree(61, 119), dict(nv=61)),
  "wave64": (lambda: _wave64(120), dict(nv=64, nbody=64, fixed=True, max_joints=2)),
  "fallbacks26": (lambda: _fallbacks(121), dict(nv=26, max_children=7, max_joints=3, child_counts=(5, 6, 7))),
  "free57": (lambda: _free_tree(57, 122), dict(nv=57)),
  "wave60": (lambda: _wave60(123), dict(nv=60, nbody=60, fixed=True, max_joints=2)),
  # the dof counts of the refused multi-tree models, on trees the engine runs
  "free21": (lambda: _free_tree(21, 124), dict(nv=21)),
  "free32": (lambda: _free_tree(32, 125), dict(nv=32)),
  "free37": (lambda: _free_tree(37, 126), dict(nv=37)),
  # non-default constraint parameters (contacts in their gap, two-sided limits)
  "params14": (lambda: _param_tree(14, 127), dict(nv=14, params=True)),
  "params38": (lambda: _param_tree(38, 128), dict(nv=38, params=True)),
}
NAMES = tuple(_RECIPES)
# Models mjx_model_create refuses ("Model shapes pinned by test"), with the
# words of its error: the engine cannot compute them yet, so they run on the oracle only.
REJECTED = {"robot_object": "a tree that follows a tree of several bodies",
            "multitree": "a tree that follows a tree of several bodies",
            "multitree_arm": "a tree that follows a tree of several bodies",
            "free61": "at most 60 dofs", "wave64": "at most 60 dofs"}
RUNNABLE = tuple(n for n in NAMES if n not in REJECTED)


def nr_for_nv(nv: int, nrs) -> int:
  """The generic register-row length for `nv` dofs: the smallest listed one that holds the
  dofs padded to a multiple of four (csrc/engine.hip generic_fn)."""
  nvp = (nv + 3) & ~3
  return min(n for n in nrs if n >= nvp)


# ----------------------------------------------------------------------------- states
def _quat_mul(a, b):
  w1, x1, y1, z1 = a
  w2, x2, y2, z2 = b
  return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                   w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def surface_heights(m, od, q):
  """[(root body, z)] of every point a colliding geom can touch the plane with at qpos `q`: a
  sphere's lowest point, both ends of a capsule (position stage of the fp64 oracle `od`)."""
  return [(r, z) for r, _, z in surface_points(m, od, q)]


def contact_thresholds(m, g):
  """The distances at which geom `g` against the plane changes what the step computes: touching,
  the contact's margin (it exists below it) and margin - gap (it has rows below it)."""
  plane = int(np.flatnonzero(np.asarray(m.geom_type) == GEOM_PLANE)[0])
  margin = max(float(m.arrays["geom_margin"][g]), float(m.arrays["geom_margin"][plane]))
  gap = max(float(m.arrays["geom_gap"][g]), float(m.arrays["geom_gap"][plane]))
  return 0.0, margin, margin - gap


def limit_distances(m, q):
  """[(joint, lower dist, upper dist, margin)] of the limited joints at qpos `q`."""
  out = []
  for j in range(m.njnt):
    if int(m.jnt_limited[j]) and int(m.jnt_type[j]) in (JNT_SLIDE, JNT_HINGE):
      x = float(q[int(m.jnt_qposadr[j])])
      lo, hi = (float(v) for v in np.asarray(m.arrays["jnt_range"])[j])
      out.append((j, x - lo, hi - x, float(m.arrays["jnt_margin"][j])))
  return out


def surface_points(m, od, q):
  """[(root body, geom, z)]: surface_heights with the geom of each point."""
  od.qpos[:] = q
  od.qvel[:] = 0.0
  od.forward()
  out = []
  gtype, gsize = np.asarray(m.geom_type), np.asarray(m.geom_size)
  for g in range(m.ngeom):
    b = int(m.geom_bodyid[g])
    if b == 0 or int(m.geom_conaffinity[g]) == 0:
      continue
    r = int(m.body_rootid[b])
    z = od.geom_xpos[g, 2] - gsize[g, 0]
    if int(gtype[g]) == GEOM_CAPSULE:
      dz = od.geom_xmat[g].reshape(3, 3)[2, 2] * gsize[g, 1]
      out += [(r, g, float(z - dz)), (r, g, float(z + dz))]
    else:
      assert int(gtype[g]) == GEOM_SPHERE, "zoo geoms are spheres and capsules"
      out.append((r, g, float(z)))
  return out


def lowest_points(m, od, q):
  """{root body: lowest z of its colliding geoms' surfaces} at qpos `q`."""
  low = {}
  for r, z in surface_heights(m, od, q):
    low[r] = min(low.get(r, np.inf), z)
  return low


@dataclass
class ZooModel:
  name: str
  model: object
  props: dict
  seed: int

  @property
  def nworld(self) -> int:
    return int(self.props.get("worlds", 16))

  def states(self, n: int | None = None):
    """Seeded (q [n, nq], qv [n, nv], ctrl [n, nu]).  Every free tree is dropped so that its
    lowest colliding surface sits between 8 mm above and 25 mm inside the plane (rows64: all
    feet down to a few lifted by the tilt), so most worlds have contacts and some have none."""
    from oracle_sim import OracleData
    m = self.model
    n = self.nworld if n is None else n
    rng = np.random.default_rng(self.seed)
    od = OracleData(m, 256, 1024)
    q0 = np.asarray(m.qpos0, float)
    q = np.tile(q0, (n, 1))
    qv = rng.normal(0.0, 0.5, (n, m.nv))
    free = []
    for j in range(m.njnt):
      a, d, t = int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j]), int(m.jnt_type[j])
      if t == JNT_FREE:
        free.append((int(m.jnt_bodyid[j]), a))
        tilt = 0.02 if self.props.get("rows64") else 0.25
        for w in range(n):
          ang = rng.normal(0.0, tilt, 3)
          th = np.linalg.norm(ang)
          q[w, a:a + 2] += rng.uniform(-0.1, 0.1, 2)
          q[w, a + 3:a + 7] = _quat_mul(q[w, a + 3:a + 7], [np.cos(th / 2), *(ang / th * np.sin(th / 2))])
        qv[:, d:d + 3] *= 0.3
      elif t == JNT_HINGE:
        q[:, a] += rng.uniform(-0.06, 0.06, n) if self.props.get("rows64") else rng.uniform(-0.5, 0.5, n)
      else:
        q[:, a] += rng.uniform(-0.08, 0.08, n)
    params = bool(self.props.get("params"))
    if params:
      # every limited joint clear of its activation distances; in every other world the joints
      # whose range is narrower than twice their margin sit where both limit rows are active
      for w in range(n):
        for j, _, _, mg in limit_distances(m, q[w]):
          a = int(m.jnt_qposadr[j])
          lo, hi = (float(v) for v in np.asarray(m.arrays["jnt_range"])[j])
          c = 2 * TIE_CLEARANCE
          if w % 2 == 0 and hi - mg + c < lo + mg - c:
            q[w, a] = rng.uniform(hi - mg + c, lo + mg - c)
          else:  # inside, within a margin, or past a limit by at most half the margin
            q[w, a] = rng.uniform(lo - 0.5 * mg, hi + 0.5 * mg)
          for _ in range(100):
            if all(abs(d - mg) > TIE_CLEARANCE for d in (q[w, a] - lo, hi - q[w, a])):
              break
            q[w, a] += 2.5 * TIE_CLEARANCE
    depth = rng.uniform(-0.008, 0.025, (n, max(len(free), 1)))
    if self.props.get("rows64"):
      depth = rng.uniform(0.0, 0.04, depth.shape)
    for w in range(n):
      low = lowest_points(m, od, q[w])
      for k, (body, a) in enumerate(free):
        if body in low:
          q[w, a + 2] -= low[body] + depth[w, k]
          if params and w % 4 == 1:  # the lowest surface point hovers in its contact's gap
            _, g, z = min((p for p in surface_points(m, od, q[w]) if p[0] == body), key=lambda p: p[2])
            _, mg, im = contact_thresholds(m, g)
            q[w, a + 2] += rng.uniform(im + 3 * TIE_CLEARANCE, mg - 3 * TIE_CLEARANCE) - z
          # keep every surface point 2e-4 clear of touching exactly: the engine's fp32 and the
          # oracle's fp64 distance must fall on the same side of the activation distance
          for _ in range(100):
            if params:  # clear of touching, of the margin and of margin - gap
              if all(abs(z - t) > TIE_CLEARANCE for r, g, z in surface_points(m, od, q[w]) if r == body
                     for t in contact_thresholds(m, g)):
                break
            elif all(abs(z) > TIE_CLEARANCE for r, z in surface_heights(m, od, q[w]) if r == body):
              break
            q[w, a + 2] -= 2.5 * TIE_CLEARANCE
    jq = np.array([m.jnt_qposadr[j] for j in m.actuator_trnid], dtype=int)
    ctrl = q[:, jq] + rng.uniform(-0.2, 0.2, (n, m.nu))
    return q, qv, ctrl


@functools.lru_cache(maxsize=None)
def get(name: str) -> ZooModel:
  make, props = _RECIPES[name]
  return ZooModel(name, make().compile(), dict(props), seed=1000 + NAMES.index(name))


def gravity_free(zm: ZooModel):
  """A contact-free, unactuated, limit-free, spring- and damper-free copy without gravity (the
  momentum route of tests/invariants.py needs a closed system)."""
  import invariants as inv
  m = inv.free_floating(zm.model, gravity=(0.0, 0.0, 0.0))
  m.arrays = dict(m.arrays)
  for k in ("jnt_stiffness", "dof_damping"):
    m.arrays[k] = np.zeros_like(m.arrays[k])
  return m


def jit_targets(name: str = "fallbacks26"):
  """(model, nconmax, njmax, role) of the run-time specialisations a default Simulation of the
  zoo model loads: its fast carve and, where it differs, its maximum carve."""
  from mjlab_amd.sim.sim import max_capacity, world_capacity
  m = copy.deepcopy(get(name).model)
  cfg = sim_cfg(m)
  cfg.mujoco.apply(m)
  fast, big = world_capacity(cfg, m), max_capacity(cfg, m)
  out = [(m, fast[0], fast[1], 1)]
  if big != fast:
    out.append((m, big[0], big[1], 2))
  return out


def sim_cfg(m, specialize: str = "never"):
  """The Simulation configuration every zoo test uses (48 contacts / 160 rows fast carve)."""
  from mjlab_amd.sim import MujocoCfg, SimulationCfg
  return SimulationCfg(nconmax=48, njmax=160, specialize=specialize,
                       mujoco=MujocoCfg(timestep=m.timestep, iterations=10, ls_iterations=20))
