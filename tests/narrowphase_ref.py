"""Independent fp64 geometry for the narrowphase tests (test infrastructure, numpy only).

Nothing here calls the oracle or restates how the oracle / the engine pick contacts: only
exact signed distances of a point to each supported shape, exact distances and closest-point
pairs between two separated shapes, and the two kinds of statement built on them that hold
for any correct narrowphase under MuJoCo's contact conventions (contact point midway
between the two surface points, normal from geom 1 to geom 2):

  (a) `check_contact`, `check_direction`: every contact has a unit normal, `dist <= margin`,
      its two surface points `pos -+ n dist / 2` on geom 1 / geom 2, and geom 2 moved along
      +n is farther;
  (b) `closest`, `check_touch_after_translation`: the deepest contact of a pair reports the
      exact distance (shapes separated, or sphere-swept shapes whose core point / segment is
      outside the other shape) or a translation that brings the shapes to touch (box-box
      penetrating, a sphere centre inside a box); test_narrowphase_pairs.check_pair applies
      them per pair.

A shape is its core (a point, a segment, a box, a plane, a triangle list) swept by a
radius.  The heightfield surface is the piecewise-linear interpolation of the elevation
grid, two triangles per cell with the diagonal p00-p11 (engine_impl.h hfield_sphere).
"""

from __future__ import annotations

import dataclasses
import itertools

import numpy as np

PLANE, HFIELD, SPHERE, CAPSULE, BOX = 0, 1, 2, 3, 6  # MuJoCo's mjtGeom values

# the code's documented bands (engine_impl.h): face / axis-kind ties, capsule-box interior
BOX_FACE_TIE = 1e-5
BOX_MID_EPS = 1e-4
MARGIN_BAND = 1e-4


def quat_mat(q):
  w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
  return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_mul(a, b):
  return np.array([a[0]*b[0]-a[1]*b[1]-a[2]*b[2]-a[3]*b[3], a[0]*b[1]+a[1]*b[0]+a[2]*b[3]-a[3]*b[2],
                   a[0]*b[2]-a[1]*b[3]+a[2]*b[0]+a[3]*b[1], a[0]*b[3]+a[1]*b[2]-a[2]*b[1]+a[3]*b[0]])


def quat_axis_angle(axis, angle):
  a = np.asarray(axis, float) / np.linalg.norm(axis)
  return np.array([np.cos(angle / 2), *(np.sin(angle / 2) * a)])


@dataclasses.dataclass
class Shape:
  kind: int
  size: np.ndarray            # MuJoCo geom size
  pos: np.ndarray             # world position
  R: np.ndarray               # world rotation (columns: the shape's axes)
  tris: np.ndarray | None = None   # hfield: (T, 3, 3) triangles in the shape's frame
  grid: tuple | None = None        # hfield: (x (ncol), y (nrow), z (nrow, ncol))

  @property
  def radius(self):
    return float(self.size[0]) if self.kind in (SPHERE, CAPSULE) else 0.0

  def local(self, p):
    return self.R.T @ (np.asarray(p, float) - self.pos)

  def world(self, p):
    return self.R @ np.asarray(p, float) + self.pos

  def moved(self, d):
    return dataclasses.replace(self, pos=self.pos + np.asarray(d, float))

  def segment(self):
    """World end points of a capsule's core segment."""
    a = self.R[:, 2] * self.size[1]
    return self.pos - a, self.pos + a

  def vertices(self):
    s = self.size[:3]
    return np.array([self.world(np.array(sg) * s) for sg in itertools.product((-1, 1), repeat=3)])

  def edges(self):
    """The box's 12 edges as world (a0, a1) pairs."""
    s, out = self.size[:3], []
    for ax in range(3):
      o1, o2 = (ax + 1) % 3, (ax + 2) % 3
      for s1, s2 in itertools.product((-1, 1), repeat=2):
        p = np.zeros(3)
        p[o1], p[o2] = s1 * s[o1], s2 * s[o2]
        lo, hi = p.copy(), p.copy()
        lo[ax], hi[ax] = -s[ax], s[ax]
        out.append((self.world(lo), self.world(hi)))
    return out


# ----------------------------------------------------------------- point to shape, shape frame
def sd_plane(p):
  return float(p[2])


def sd_sphere(p, r):
  return float(np.linalg.norm(p) - r)


def sd_capsule(p, r, h):
  c = np.array([0.0, 0.0, np.clip(p[2], -h, h)])
  return float(np.linalg.norm(p - c) - r)


def sd_box(p, s):
  d = np.abs(p) - s
  return float(np.linalg.norm(np.maximum(d, 0.0)) + min(d.max(), 0.0))


def hfield_triangles(data, size):
  """(tris, grid) of a heightfield: data (nrow, ncol) in [0, 1] (row = y, column = x), size
  (sx, sy, sz, base); two triangles per cell, p00 p10 p11 and p00 p11 p01."""
  data = np.asarray(data, float)
  nr, nc = data.shape
  x = np.linspace(-size[0], size[0], nc)
  y = np.linspace(-size[1], size[1], nr)
  z = data * size[2]
  tris = []
  for r in range(nr - 1):
    for c in range(nc - 1):
      p00, p10 = (x[c], y[r], z[r, c]), (x[c + 1], y[r], z[r, c + 1])
      p01, p11 = (x[c], y[r + 1], z[r + 1, c]), (x[c + 1], y[r + 1], z[r + 1, c + 1])
      tris += [(p00, p10, p11), (p00, p11, p01)]
  return np.array(tris, float), (x, y, z)


def closest_on_triangles(p, tris):
  """Closest point of each triangle (T, 3, 3) to p: the projection onto the plane where it
  falls inside, else the nearest of the three edges' closest points."""
  a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
  n = np.cross(b - a, c - a)
  n /= np.linalg.norm(n, axis=1, keepdims=True)
  pp = p - n * np.einsum("ij,ij->i", p - a, n)[:, None]
  inside = np.ones(len(tris), bool)
  best = np.full(len(tris), np.inf)
  q = np.zeros_like(a)
  for s0, s1 in ((a, b), (b, c), (c, a)):
    inside &= np.einsum("ij,ij->i", np.cross(s1 - s0, pp - s0), n) >= 0.0
    e = s1 - s0
    t = np.clip(np.einsum("ij,ij->i", p - s0, e) / np.einsum("ij,ij->i", e, e), 0.0, 1.0)
    cp = s0 + e * t[:, None]
    d = np.linalg.norm(p - cp, axis=1)
    take = d < best
    best = np.where(take, d, best)
    q[take] = cp[take]
  q[inside] = pp[inside]
  return q


def hfield_height(grid, x, y):
  """Surface height over (x, y), or None outside the grid."""
  gx, gy, gz = grid
  if not (gx[0] <= x <= gx[-1] and gy[0] <= y <= gy[-1]):
    return None
  c = min(int(np.searchsorted(gx, x, side="right")) - 1, len(gx) - 2)
  r = min(int(np.searchsorted(gy, y, side="right")) - 1, len(gy) - 2)
  fx, fy = (x - gx[c]) / (gx[c + 1] - gx[c]), (y - gy[r]) / (gy[r + 1] - gy[r])
  z00, z10, z01, z11 = gz[r, c], gz[r, c + 1], gz[r + 1, c], gz[r + 1, c + 1]
  if fy <= fx:
    return z00 + fx * (z10 - z00) + fy * (z11 - z10)
  return z00 + fy * (z01 - z00) + fx * (z11 - z01)


def hfield_closest(p, tris):
  """(distance, closest surface point, unique) of p to the triangle list."""
  q = closest_on_triangles(p, tris)
  d = np.linalg.norm(q - p, axis=1)
  k = int(np.argmin(d))
  near = d < d[k] + 1e-9
  unique = bool(np.linalg.norm(q[near] - q[k], axis=1).max() < 1e-7)
  return float(d[k]), q[k], unique


def sd_hfield(p, tris, grid):
  d = hfield_closest(p, tris)[0]
  h = hfield_height(grid, p[0], p[1])
  return -d if h is not None and p[2] < h else d


def signed_distance(shape: Shape, pw):
  """Exact signed distance of the world point pw to the shape (negative inside)."""
  p = shape.local(pw)
  if shape.kind == PLANE:
    return sd_plane(p)
  if shape.kind == SPHERE:
    return sd_sphere(p, shape.size[0])
  if shape.kind == CAPSULE:
    return sd_capsule(p, shape.size[0], shape.size[1])
  if shape.kind == BOX:
    return sd_box(p, shape.size[:3])
  if shape.kind == HFIELD:
    return sd_hfield(p, shape.tris, shape.grid)
  raise ValueError(shape.kind)


# ----------------------------------------------------------------- core to core, world frame
def point_segment(p, a0, a1):
  e = a1 - a0
  ee = float(e @ e)
  t = 0.0 if ee == 0.0 else float(np.clip((p - a0) @ e / ee, 0.0, 1.0))
  q = a0 + e * t
  return float(np.linalg.norm(p - q)), q


def segment_segment(a0, a1, b0, b1):
  """(distance, pa, pb, unique): the interior stationary point where both parameters fall in
  [0, 1], and every end point against the other segment; the least of them."""
  cand = []
  u, v, w = a1 - a0, b1 - b0, a0 - b0
  a, b, c, d, e = u @ u, u @ v, v @ v, u @ w, v @ w
  den = a * c - b * b
  if den > 1e-14 * a * c:
    s, t = (b * e - c * d) / den, (a * e - b * d) / den
    if 0.0 <= s <= 1.0 and 0.0 <= t <= 1.0:
      cand.append((a0 + u * s, b0 + v * t))
  for p in (a0, a1):
    cand.append((p, point_segment(p, b0, b1)[1]))
  for p in (b0, b1):
    cand.append((point_segment(p, a0, a1)[1], p))
  dist = np.array([np.linalg.norm(pa - pb) for pa, pb in cand])
  k = int(np.argmin(dist))
  near = [i for i in range(len(cand)) if dist[i] < dist[k] + 1e-9]
  unique = all(np.linalg.norm(cand[i][0] - cand[k][0]) < 1e-7 for i in near)
  return float(dist[k]), cand[k][0], cand[k][1], unique


def point_box(p, box: Shape):
  """(signed distance, nearest box surface point when outside)."""
  q = box.local(p)
  s = box.size[:3]
  return sd_box(q, s), box.world(np.clip(q, -s, s))


def segment_box_distance(c, a, hl, s):
  """min over the segment c + t a (|t| <= hl) of the box signed distance (box frame, half
  sizes s), fp64: dense samples, then golden refinement in the best bracket; returns
  (distance, t) -- an oracle-independent restatement of what MuJoCo's first capsule-box
  contact reports (the sphere at the segment point closest to the box)."""
  def sd(t):
    q = c[None, :] + np.atleast_1d(t)[:, None] * a[None, :]
    d = np.abs(q) - s
    out = np.linalg.norm(np.maximum(d, 0.0), axis=1) + np.minimum(d.max(axis=1), 0.0)
    return out
  ts = np.linspace(-hl, hl, 4001)
  v = sd(ts)
  k = int(np.argmin(v))
  lo, hi = ts[max(k - 1, 0)], ts[min(k + 1, len(ts) - 1)]
  for _ in range(80):
    m1, m2 = lo + (hi - lo) * 0.382, lo + (hi - lo) * 0.618
    if sd(m1)[0] <= sd(m2)[0]:
      hi = m2
    else:
      lo = m1
  t = 0.5 * (lo + hi)
  cand = [(float(sd(t)[0]), t), (float(v[k]), ts[k])]
  return min(cand)


def segment_box(cap: Shape, box: Shape):
  """(signed distance of the segment's nearest point, that point, the box point nearest it,
  unique, distance of the nearer segment end)."""
  c, a = box.local(cap.pos), box.R.T @ cap.R[:, 2]
  hl, s = float(cap.size[1]), box.size[:3]
  d, t = segment_box_distance(c, a, hl, s)
  ts = np.linspace(-hl, hl, 4001)
  q = c[None, :] + ts[:, None] * a[None, :]
  dd = np.abs(q) - s
  v = np.linalg.norm(np.maximum(dd, 0.0), axis=1) + np.minimum(dd.max(axis=1), 0.0)
  flat = ts[v < d + 1e-9]
  unique = len(flat) == 0 or flat.max() - flat.min() < 3 * (ts[1] - ts[0])
  pl = c + a * t
  ends = min(sd_box(c - a * hl, s), sd_box(c + a * hl, s))
  return d, box.world(pl), box.world(np.clip(pl, -s, s)), bool(unique), ends


def _segments_closest(a0, a1, b0, b1):
  """segment_segment for arrays of segments (N, 3): (distance (N), pa, pb)."""
  def pt_seg(p, s0, s1):
    e = s1 - s0
    t = np.clip(np.einsum("ij,ij->i", p - s0, e) / np.einsum("ij,ij->i", e, e), 0.0, 1.0)
    return s0 + e * t[:, None]
  u, v, w = a1 - a0, b1 - b0, a0 - b0
  dot = lambda x, y: np.einsum("ij,ij->i", x, y)
  a, b, c, d, e = dot(u, u), dot(u, v), dot(v, v), dot(u, w), dot(v, w)
  den = a * c - b * b
  ok = den > 1e-14 * a * c
  sden = np.where(ok, den, 1.0)
  s, t = (b * e - c * d) / sden, (a * e - b * d) / sden
  ok &= (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
  cand = [(a0 + u * s[:, None], b0 + v * t[:, None], ok)]
  yes = np.ones(len(a0), bool)
  cand += [(a0, pt_seg(a0, b0, b1), yes), (a1, pt_seg(a1, b0, b1), yes),
           (pt_seg(b0, a0, a1), b0, yes), (pt_seg(b1, a0, a1), b1, yes)]
  best = np.full(len(a0), np.inf)
  pa, pb = np.zeros_like(a0), np.zeros_like(a0)
  for qa, qb, valid in cand:
    dist = np.where(valid, np.linalg.norm(qa - qb, axis=1), np.inf)
    take = dist < best
    best = np.where(take, dist, best)
    pa[take], pb[take] = qa[take], qb[take]
  return best, pa, pb


def _edge_pierces(a0, a1, box: Shape, eps=1e-13):
  """Whether the segment a0 a1 passes through the box's interior (slab clipping in the box
  frame, the box shrunk by eps)."""
  p, e = box.local(a0), box.R.T @ (a1 - a0)
  s = box.size[:3] - eps
  t0, t1 = 0.0, 1.0
  for i in range(3):
    if abs(e[i]) < 1e-300:
      if abs(p[i]) >= s[i]:
        return False
      continue
    ta, tb = (-s[i] - p[i]) / e[i], (s[i] - p[i]) / e[i]
    t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
  return t1 - t0 > 0.0


def boxes_overlap(A: Shape, B: Shape):
  """Two convex polyhedra share interior points exactly when an edge of one passes through
  the other's interior."""
  return (any(_edge_pierces(a0, a1, B) for a0, a1 in A.edges()) or
          any(_edge_pierces(b0, b1, A) for b0, b1 in B.edges()))


def box_box(A: Shape, B: Shape):
  """(distance, pa, pb, unique) of two boxes: the least of the vertex-to-box distances (both
  ways) and the 144 edge-edge segment distances; -1 when the boxes overlap."""
  if boxes_overlap(A, B):
    return -1.0, A.pos, B.pos, False
  cand = []
  for v in A.vertices():
    d, q = point_box(v, B)
    cand.append((d, v, q))
  for v in B.vertices():
    d, q = point_box(v, A)
    cand.append((d, q, v))
  ea, eb = A.edges(), B.edges()
  idx = [(i, j) for i in range(12) for j in range(12)]
  a0 = np.array([ea[i][0] for i, _ in idx]); a1 = np.array([ea[i][1] for i, _ in idx])
  b0 = np.array([eb[j][0] for _, j in idx]); b1 = np.array([eb[j][1] for _, j in idx])
  de, pa, pb = _segments_closest(a0, a1, b0, b1)
  cand += [(float(de[k]), pa[k], pb[k]) for k in range(len(idx))]
  dist = np.array([c[0] for c in cand])
  k = int(np.argmin(dist))
  near = [c for c in cand if c[0] < dist[k] + 1e-9]
  unique = all(np.linalg.norm(c[1] - cand[k][1]) < 1e-7 and np.linalg.norm(c[2] - cand[k][2]) < 1e-7
               for c in near)
  return float(dist[k]), cand[k][1], cand[k][2], unique


@dataclasses.dataclass
class Closest:
  dist: float           # exact distance of the shapes (core distance minus the radii)
  core: float           # signed distance of the cores (<= 0: the cores meet)
  pa: np.ndarray        # surface point of shape A
  pb: np.ndarray        # surface point of shape B
  n: np.ndarray         # direction from A toward B
  unique: bool          # the closest-point pair is unique
  ends: float | None = None   # capsule-box: the nearer segment end's core distance


def closest(A: Shape, B: Shape) -> Closest:
  """Exact distance and closest-point pair of shape A to shape B, A's kind <= B's (MuJoCo's
  pair order).  Valid while the cores are apart (`core > 0`)."""
  ka, kb = A.kind, B.kind
  ends = None
  if ka == PLANE:
    n = A.R[:, 2]
    if kb == SPHERE:
      pts = [B.pos]
    elif kb == CAPSULE:
      pts = list(B.segment())
    else:
      pts = list(B.vertices())
    h = np.array([(p - A.pos) @ n for p in pts])
    k = int(np.argmin(h))
    unique = bool((np.sort(h)[1] > h[k] + 1e-9) if len(h) > 1 else True)
    cb, core = pts[k], float(h[k])
    ca, u = cb - n * core, n
  elif ka == HFIELD:
    pts = [B.pos] if kb == SPHERE else list(B.segment())
    res = [hfield_closest(A.local(p), A.tris) for p in pts]
    sgn = [-1.0 if signed_distance(A, p) < 0 else 1.0 for p in pts]
    k = int(np.argmin([r[0] * g for r, g in zip(res, sgn)]))
    core, q, unique = res[k]
    core *= sgn[k]
    ca, cb = A.world(q), pts[k]
    u = (cb - ca) / max(abs(core), 1e-300)
  else:
    if ka == SPHERE and kb == SPHERE:
      ca, cb, unique = A.pos, B.pos, True
      core = float(np.linalg.norm(cb - ca))
    elif ka == SPHERE and kb == CAPSULE:
      core, cb = point_segment(A.pos, *B.segment())
      ca, unique = A.pos, True
    elif ka == CAPSULE and kb == CAPSULE:
      core, ca, cb, unique = segment_segment(*A.segment(), *B.segment())
    elif ka == SPHERE and kb == BOX:
      core, cb = point_box(A.pos, B)
      ca, unique = A.pos, True
    elif ka == CAPSULE and kb == BOX:
      core, ca, cb, unique, ends = segment_box(A, B)
    elif ka == BOX and kb == BOX:
      core, ca, cb, unique = box_box(A, B)
    else:
      raise ValueError((ka, kb))
    u = (cb - ca) / max(float(np.linalg.norm(cb - ca)), 1e-300)
  if core <= 0:
    unique = False
  return Closest(core - A.radius - B.radius, core, ca + u * A.radius, cb - u * B.radius, u,
                 bool(unique), ends)


# ----------------------------------------------------------------- the two statements
DELTA = 1e-3  # (a): geom 2 moved this far along +n


def check_contact(A: Shape, B: Shape, con, margin, tol, ntol=1e-9, surface=(True, True)):
  """(a) for one contact row (g1, g2, dist, pos[3], n[3]).  `surface`: whether the point on
  geom 1 / geom 2 must lie on the surface; where False (a capsule's sphere contact whose
  normal leaves the cap, see check rules in test_narrowphase_pairs) it must not lie outside."""
  dist, pos, n = float(con[2]), np.asarray(con[3:6], float), np.asarray(con[6:9], float)
  assert abs(np.linalg.norm(n) - 1.0) <= ntol, f"|n| = {np.linalg.norm(n)}"
  assert dist <= margin + tol, f"dist {dist} > margin {margin}"
  for S, p, on, name in ((A, pos - n * dist / 2, surface[0], "geom 1"),
                         (B, pos + n * dist / 2, surface[1], "geom 2")):
    sd = signed_distance(S, p)
    if on:
      assert abs(sd) <= tol, f"point on {name}: signed distance {sd}"
    else:
      assert sd <= tol, f"point on {name}: outside by {sd}"


def check_direction(A: Shape, B: Shape, con, tol, depth=None):
  """(a), the normal's sense: geom 2 moved by +n DELTA is farther (cores apart, or a plane),
  or, moved by the pair's depth + DELTA, is separated (cores overlapping)."""
  dist, n = float(con[2] if depth is None else depth), np.asarray(con[6:9], float)
  c0 = closest(A, B)
  if c0.core > 0 or A.kind == PLANE:
    c1 = closest(A, B.moved(n * DELTA))
    assert c1.dist > c0.dist + 1e-3 * DELTA, f"moving geom 2 along n: {c0.dist} -> {c1.dist}"
  else:
    c1 = closest(A, B.moved(n * (abs(dist) + DELTA)))
    assert c1.core > 0 and c1.dist > 0.5 * DELTA - tol, f"pushed out along n: distance {c1.dist}"


def check_touch_after_translation(A: Shape, B: Shape, con, tol):
  """(b), cores overlapping: geom 2 moved by |dist| n touches geom 1 -- moved by tol more
  the shapes are apart, by no more than 2 tol; moved by tol less they are not."""
  dist, n = float(con[2]), np.asarray(con[6:9], float)
  hi = closest(A, B.moved(n * (abs(dist) + tol))).dist
  lo = closest(A, B.moved(n * (abs(dist) - tol))).dist
  assert -1e-12 <= hi <= 2 * tol + 1e-12, f"moved by |dist| + {tol}: distance {hi}"
  assert lo <= 1e-12, f"moved by |dist| - {tol}: still apart by {lo}"
