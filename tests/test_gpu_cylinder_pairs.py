"""Cylinder narrowphase on the GPU against the exact fp64 geometry of cylinder_ref.

One scene per pair kind: two free cylinders (r 0.05, h 0.12 and the disk r 0.1, h 0.01; the unused
one parked 3 m away) and one partner: the plane, a free sphere, capsule, cylinder or box, or a box
welded to the world (the terrain loop).  64 worlds, one fp32 pose each, `forward()` only.  A pose is
an orientation and a start point, moved along the exact closest-point direction to its gap: beyond
the margin, inside it, or overlapping by at most 0.1 r; the CONSTRUCTED poses come first.  Bounds:
D_TOL / N_TOL of test_gpu_narrowphase_pairs.py plus 4 x the *_MEASURED constants (engine minus
cylinder_ref over these seeds, one MI355X, generic kernels; printed), capped at kBoxMidEps."""

import collections
import functools
import types

import numpy as np
import pytest
import torch

import cylinder_ref as C
import narrowphase_ref as R
import test_narrowphase_pairs as P
from cylinder_ref import CYLINDER
from narrowphase_ref import BOX, CAPSULE, PLANE, SPHERE

pytestmark = pytest.mark.gpu

KINDS = ("plane", "sphere", "capsule", "cylinder", "box", "terrain_box")
CONVEX = ("cylinder", "box", "terrain_box")
NW, MARGIN = 64, P.MARGIN
D_TOL, N_TOL, EPS32 = 2e-6, 2e-5, 2.0 ** -23
CAPSULE_POS_MEASURED = 4.28e-5  # capsule, apart: |pos - exact| of the deepest contact inside the segment
CONVEX_DIST_MEASURED = 6.95e-8  # convex pairs: |dist - exact| apart, |-dist - depth along n| overlapping
CONVEX_SURF_MEASURED = 2.2e-6   # convex pairs: distance of either surface point to its shape
CONVEX_N_MEASURED = 2.06e-5     # convex pairs, apart: |n - exact direction|
DEPTH_RATIO_MEASURED = 1.09     # convex pairs, overlapping: reported depth / minimal depth (box)
CAPSULE_POS, CONVEX_DIST, CONVEX_SURF, CONVEX_N = (min(4 * x, R.BOX_MID_EPS) for x in (
  CAPSULE_POS_MEASURED, CONVEX_DIST_MEASURED, CONVEX_SURF_MEASURED, CONVEX_N_MEASURED))
CYL_MID_EPS = 1e-6  # engine_impl.h kCylMidEps: the capsule's interior contact is kept when deeper by this

SIZES = ((0.05, 0.12), (0.1, 0.01))
PARTNER = {"sphere": ("sphere", (0.06,)), "capsule": ("capsule", (0.04, 0.15)),
           "cylinder": ("cylinder", (0.07, 0.09)), "box": ("box", (0.12, 0.1, 0.06))}
I, X90, Y45 = P.IDENT, R.quat_axis_angle((1, 0, 0), np.pi / 2), R.quat_axis_angle((0, 1, 0), np.pi / 4)
PEN = -0.002  # gap of the overlapping constructed poses
# (cylinder quat, start centre in the partner's frame: units of (r, r, h) plus an offset, gap or None =
# as placed).  Plane: upright, lying, tilted rim.  Sphere: on the axis beyond a cap, inside, beyond a rim.
# Capsule / cylinder: along the side, across a cap / stacked, crossed.  Boxes: flat, lying, rim on an edge.
UP, SIDE, TOP = ((0, 0, 0), (0, 0, 1)), ((0, 0, 0), (0.5, 0, 0.02)), ((0, 0, 0), (0.02, 0.01, 0.5))
_BOX = [(I, TOP, PEN), (X90, TOP, PEN), (Y45, "edge", PEN), (Y45, "edge", 0.5 * MARGIN)]
CONSTRUCTED = {
  "plane": [(I, UP, PEN), (X90, UP, PEN), (Y45, UP, PEN)],
  "sphere": [(I, UP, PEN), (I, ((0, 0, -0.3), (0, 0, 0)), None), (I, ((0, 0, 0.3), (0, 0, 0)), None),
             (I, ((1, 0, 1), (0.2, 0, 0.2)), PEN)],
  "capsule": [(I, SIDE, PEN), (X90, ((0, 0, 0), (0.01, 0, 0.5)), PEN), (X90, SIDE, 0.5 * MARGIN)],
  "cylinder": [(I, SIDE, PEN), (I, TOP, PEN), (X90, ((0, 0, 0), (0.5, 0, 0.01)), PEN)],
  "box": _BOX, "terrain_box": _BOX}


@functools.lru_cache(maxsize=None)
def model(kind):
  bodies = [P._free("c", "cylinder", SIZES[0]), P._free("d", "cylinder", SIZES[1])]
  ent = P.EntitySpec("pair", P._mjcf(bodies + ([P._free("p", *PARTNER[kind])] if kind in PARTNER else [])))
  if kind == "terrain_box":
    box = P.BoxSpec("terrain_0", pos=tuple(P.ST_POS), size=tuple(P.ST_SIZE))
    return P.compile_scene([ent], terrain="generator", terrain_geoms=[box], timestep=0.005)
  return P.compile_scene([ent], terrain="plane" if kind == "plane" else "none", timestep=0.005)


def pair_of(m, sh, w):
  """Geom ids of world w's pair: (geom 1, geom 2) by type, then (probe cylinder, partner)."""
  cyl = [g for g in range(m.ngeom) if int(m.geom_type[g]) == CYLINDER][:2]
  part = [g for g in range(m.ngeom) if g not in cyl][0]
  return sorted((cyl[w % 2], part), key=lambda g: (sh[g].kind, g)), (cyl[w % 2], part)


@functools.lru_cache(maxsize=None)
def poses(kind):
  """(NW, nq) qpos, fp32-representable.  World w uses cylinder w % 2."""
  m, rng = model(kind), np.random.default_rng(KINDS.index(kind) + 11)
  q = np.zeros((NW, 21 if kind in PARTNER else 14))
  for w in range(NW):
    (k, i), (r, h) = (w % 2, w // 2), SIZES[w % 2]
    made = i < len(CONSTRUCTED[kind])
    q[w, 3::7] = 1.0
    q[w, 7 * (1 - k):7 * (1 - k) + 3] = 3.0  # parked
    fp, fq = (P.ST_POS, I) if kind == "terrain_box" else (np.zeros(3), I)
    if kind in PARTNER:
      fp, fq = (fp, fq) if made else (P.FX_POS, P.FX_QUAT)
      q[w, 14:17], q[w, 17:21] = fp, fq
    if made:
      qc, p0, gap = CONSTRUCTED[kind][i]
      if p0 == "edge":  # the lowest rim point over the box edge
        s = P.ST_SIZE if kind == "terrain_box" else PARTNER["box"][1]
        low = C.support(R.Shape(CYLINDER, np.array(SIZES[k]), np.zeros(3), R.quat_mat(Y45)), (0, 0, -1))
        p0 = np.array([s[0] - low[0], 0.01, 0.5])
      else:
        p0 = np.array(p0[0]) * (r, r, h) + p0[1]
    else:
      qc, u = rng.normal(size=4), rng.normal(size=3)
      u = np.array([0.3 * u[0], 0.3 * u[1], 1.0]) if kind == "plane" else u
      p0 = 0.8 * u / np.linalg.norm(u)
      gap = (MARGIN + rng.uniform(0.002, 0.03), rng.uniform(0.1, 0.9) * MARGIN, -rng.uniform(0.02, 0.1) * r)[i % 3]
    q[w, 7 * k:7 * k + 3] = fp + R.quat_mat(fq) @ p0
    q[w, 7 * k + 3:7 * k + 7] = R.quat_mul(fq, qc / np.linalg.norm(qc))
    q[w] = q[w].astype(np.float32)
    if gap is not None:
      sh = P.shapes(m, q[w])
      probe, part = pair_of(m, sh, w)[1]
      d, _, _, n = C.closest(sh[part], sh[probe])
      q[w, 7 * k:7 * k + 3] -= n * (d - gap)
      q[w] = q[w].astype(np.float32)
  return q


def exact(A, B):
  """(signed distance, whether exact, direction, contact point).  Overlapping: closed form for plane and
  sphere, the capsule's segment sampled (second order, < 1e-7), convex pairs minus the minimal depth."""
  d, pa, pb, n = C.closest(A, B)
  if d > 0:
    return d, True, n, (pa + pb) / 2
  if A.kind == PLANE:
    return -C.directional_depth(A, B, A.R[:, 2]), True, None, None
  if A.kind in (SPHERE, CAPSULE):
    ts = np.linspace(-A.size[1], A.size[1], 2001) if A.kind == CAPSULE else [0.0]
    return min(C.signed_distance(B, A.pos + A.R[:, 2] * t) for t in ts) - A.size[0], True, None, None
  return -C.minimal_depth(A, B)[0], False, None, None


@functools.lru_cache(maxsize=None)
def references(kind):
  """Per world (A, B, pair, exact(A, B), class), with the pose shares checked: reference only."""
  m, q, out = model(kind), poses(kind), []
  for w in range(NW):
    sh = P.shapes(m, q[w])
    pair = pair_of(m, sh, w)[0]
    ex = exact(sh[pair[0]], sh[pair[1]])
    cls = ("band" if abs(ex[0] - MARGIN) <= R.MARGIN_BAND else "out" if ex[0] > MARGIN else "near" if ex[0] > 0
           else "pen" if ex[0] >= -0.1 * SIZES[w % 2][0] - 1e-7 else "deep")
    out.append((sh[pair[0]], sh[pair[1]], pair, ex, cls))
  share = collections.Counter(o[4] for o in out)
  assert share["band"] <= 0.05 * NW and min(share["out"], share["near"], share["pen"]) >= NW // 4, share
  return out


def check(kind, eng):
  conv, cap = kind in CONVEX, kind == "capsule"
  dtol = D_TOL + (CONVEX_DIST if conv else CYL_MID_EPS if cap else 0.0)
  stol = D_TOL + (CONVEX_SURF if conv else 0.0)
  worst, fails = collections.Counter(), []
  for w, (A, B, pair, (sd, ex, n, mp), cls) in enumerate(references(kind)):
    cons = eng[w]
    try:
      assert cls != "out" or len(cons) == 0, f"{len(cons)} contacts at exact distance {sd:.6g} > margin"
      if cls in ("band", "out"):
        continue
      assert len(cons) >= 1 and np.array_equal(cons[:, :2], np.tile(pair, (len(cons), 1))), f"geoms {cons[:, :2].tolist()}"
      if kind == "plane" and w < 6:  # upright, lying, tilted rim; the disk (2 h = margin) adds its far rim
        assert len(cons) == ((3, 4), (2, 2), (1, 2))[w // 2][w % 2], f"{len(cons)} contacts"
      deep = int(np.argmin(cons[:, 2]))
      for i, (dist, pos, nn) in enumerate((c[2], c[3:6], c[6:9]) for c in cons):
        assert abs(np.linalg.norm(nn) - 1) <= N_TOL and dist <= MARGIN + D_TOL, f"|n|, dist {dist}"
        # (a capsule's second sphere may touch its own capsule from inside: not outside, then)
        for S, pt, on in ((A, pos - nn * dist / 2, not cap or i == deep), (B, pos + nn * dist / 2, True)):
          e = abs(C.signed_distance(S, pt)) if on else max(C.signed_distance(S, pt), 0.0)
          worst["surf"] = max(worst["surf"], e)
          assert e <= stol, f"contact {i}: surface point off geom kind {S.kind} by {e:.3g}"
      dist, pos, nn = cons[deep, 2], cons[deep, 3:6], cons[deep, 6:9]
      ref = sd if ex else -C.directional_depth(A, B, nn)  # (convex, overlapping: the depth along n)
      worst["dist"], worst["ratio"] = max(worst["dist"], abs(dist - ref)), max(worst["ratio"], 0.0 if ex else dist / sd)
      assert abs(dist - ref) <= dtol, f"dist {dist:.9g} vs {ref:.9g}"
      if n is not None and sd + A.radius > 4 * EPS32:
        mid = cap and abs((pos - nn * (dist / 2 + A.size[0]) - A.pos) @ A.R[:, 2]) < A.size[1] - 1e-6
        ptol = CAPSULE_POS if mid else 0.0  # the golden-section search's position, and its turn of n
        ep, en = np.abs(pos - mp).max() if mid else 0.0, np.abs(nn - n).max()
        worst["mid_pos"], worst["normal"] = max(worst["mid_pos"], ep), max(worst["normal"], en)
        assert ep <= D_TOL + ptol, f"interior contact off by {ep:.3g}"
        assert en <= N_TOL + (CONVEX_N if conv else ptol / (sd + A.radius)), f"normal off by {en:.3g}"
    except AssertionError as exn:
      fails.append(f"world {w}: {exn}")
  print(f"\n[cylinder {kind}] maxima: " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
  assert not fails and worst["ratio"] <= 1.5 * DEPTH_RATIO_MEASURED, f"{kind}: {len(fails)} failures\n" + "\n".join(fails[:12])


@pytest.mark.parametrize("kind", KINDS)
def test_cylinder_pair_against_exact_geometry(kind, gpu_device):
  import test_gpu_narrowphase_pairs as G
  references(kind)  # the pose shares, before anything runs on the GPU
  # (engine_contacts asserts unsupported == 0, which an engine without cylinders fails, and con_overflow == 0)
  check(kind, G.engine_contacts(types.SimpleNamespace(model=model(kind)), poses(kind).astype(np.float32), gpu_device))


@functools.lru_cache(maxsize=None)
def step_scene():
  from mjlab_amd.sim import MujocoCfg, SimulationCfg
  ent = P.EntitySpec("pair", P._mjcf([P._free("c", "cylinder", (0.05, 0.12)), P._free("b", "box", (0.05, 0.05, 0.12))]))
  cfg = SimulationCfg(nconmax=16, njmax=64, mujoco=MujocoCfg(timestep=0.005, iterations=20, ls_iterations=20))
  return P.compile_scene([ent], terrain="plane", timestep=0.005), cfg


def jit_targets():
  from mjlab_amd.sim.sim import max_capacity, world_capacity  # (build() compiles these (model, ncon, rows, role))
  m, cfg = step_scene()
  fast, big = world_capacity(cfg, m), max_capacity(cfg, m)
  return [(m, *fast, 1)] + ([(m, *big, 2)] if big != fast else [])


@pytest.mark.parametrize("specialize", ["never", "always"])
def test_upright_cylinder_rests_like_a_box(specialize, gpu_device):
  """One step() of an upright cylinder and a box of its mass and half-height: generic and JIT kernels."""
  import dataclasses
  from mjlab_amd.sim import Simulation
  m, cfg = step_scene()
  sim = Simulation(4, dataclasses.replace(cfg, specialize=specialize), m, gpu_device)
  assert (sim.info()["spec"] > 0) == (specialize == "always"), sim.info()
  d, q = sim.data, np.zeros((4, 14), np.float32)
  q[:, 3::7], q[:, 2::7], q[:, 7] = 1.0, 0.12 - 0.001, 1.0
  d.qpos[:] = torch.as_tensor(q)
  d.qvel.zero_()
  d.qacc_warmstart.zero_()
  sim.step()
  torch.cuda.synchronize()
  st, ncon, nefc = sim.stats(), *(x.cpu().numpy().reshape(4) for x in (d.ncon, d.nefc))
  assert np.array_equal(ncon, [7] * 4) and np.array_equal(nefc, 4 * ncon), (ncon, nefc)  # pyramidal, condim 3
  assert torch.isfinite(d.qacc).all() and st["unsupported"] == 0 and st["con_overflow"] == 0, st
  geom = d.contact_geom.reshape(4, -1, 2).cpu().numpy()
  fn = d.contact_force.reshape(4, -1, 3).cpu().numpy()[..., 0]
  gt, mg = np.asarray(m.geom_type), 9.81 * 1.0
  for w in range(4):
    f = {t: fn[w, :ncon[w]][gt[geom[w, :ncon[w], 1]] == t].sum() for t in (CYLINDER, BOX)}
    print(f"[cylinder step] world {w}: normal force cylinder {f[CYLINDER]:.6g} box {f[BOX]:.6g} m g {mg:.6g}")
    assert abs(f[CYLINDER] - f[BOX]) <= 2 * abs(f[BOX] - mg), f
