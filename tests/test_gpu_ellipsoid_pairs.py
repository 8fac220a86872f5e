"""Ellipsoid narrowphase on the GPU against the exact fp64 geometry of ellipsoid_ref, laid out as
test_gpu_cylinder_pairs.py (whose pose constants it shares): two free probe ellipsoids (tri-axial, and a
10:1 disc; the unused one parked 3 m away) and one partner per scene, 64 worlds, `forward()` only; poses
moved along the exact closest direction to a gap beyond the margin, inside it, or overlapping by at most
0.1 x the smallest semi-axis, the CONSTRUCTED ones first.  Bounds: D_TOL / N_TOL plus 4 x the *_MEASURED
constants (engine minus ellipsoid_ref over these seeds, one MI355X, generic kernels), capped at kBoxMidEps."""

import collections
import functools
import types

import numpy as np
import pytest
import torch

import ellipsoid_ref as E
import narrowphase_ref as R
import test_narrowphase_pairs as P
from ellipsoid_ref import ELLIPSOID
from narrowphase_ref import PLANE, SPHERE
from test_gpu_cylinder_pairs import D_TOL, EPS32, I, MARGIN, N_TOL, NW, PEN, SIDE, TOP, UP, X90, Y45, _BOX

pytestmark = pytest.mark.gpu

KINDS = ("plane", "sphere", "capsule", "ellipsoid", "cylinder", "box", "terrain_box")
CONVEX = KINDS[2:]  # through convex_pair
SPHERE_MEASURED = 1.23e-7        # sphere (the fp32 root-finder): |dist - exact|, either surface point off its shape
SPHERE_N_MEASURED = 4.27e-7      # sphere, apart: |n - exact direction|
CONVEX_DIST_MEASURED = 7.39e-8   # convex pairs: |dist - exact| apart, |-dist - depth along n| overlapping
CONVEX_SURF_MEASURED = 2.56e-5   # convex pairs: distance of either surface point to its shape
CONVEX_N_MEASURED = 2.94e-5      # convex pairs, apart: |n - exact direction|
DEPTH_RATIO_MEASURED = 1.00      # convex pairs, overlapping: reported depth / minimal depth
SPHERE_TOL, SPHERE_N, CONVEX_DIST, CONVEX_SURF, CONVEX_N = (min(4 * x, R.BOX_MID_EPS) for x in (
  SPHERE_MEASURED, SPHERE_N_MEASURED, CONVEX_DIST_MEASURED, CONVEX_SURF_MEASURED, CONVEX_N_MEASURED))

SIZES = ((0.05, 0.08, 0.12), (0.1, 0.1, 0.01))
PARTNER = {"sphere": ("sphere", (0.06,)), "capsule": ("capsule", (0.04, 0.15)), "ellipsoid": ("ellipsoid", (0.09, 0.04, 0.06)),
           "cylinder": ("cylinder", (0.07, 0.09)), "box": ("box", (0.12, 0.1, 0.06))}
# closest()'s alternating projections stop at steps of 1e-14: between overlapping smooth shapes (a thin lens)
# that can be at a distance of 1e-9 rather than below its own 1e-10, so anything nearer than this overlaps
TOUCH = 1e-8
# (ellipsoid quat, start centre in the partner's frame: units of the semi-axes plus an offset, gap or None = as
# placed).  On the z axis (the flat of the disc), on the y axis, tilted, over a box edge.  The sphere's centre
# inside the ellipsoid: on an axis, at the centre, and in the smallest axis' symmetry plane where the pole's
# stationary point exists (0 0.3 0) and, past it near the rim, for the tri-axial probe and for the disc.
_IN = lambda *u: (I, (u, (0, 0, 0)), None)
_PAIR = [(I, UP, PEN), (X90, UP, PEN), (I, SIDE, PEN), (Y45, SIDE, 0.5 * MARGIN)]
CONSTRUCTED = {
  "plane": [(I, UP, PEN), (X90, UP, PEN), (Y45, UP, PEN)],
  "sphere": [(I, UP, PEN), (X90, UP, 0.5 * MARGIN), _IN(0, 0, 0.5), _IN(0, 0, 0), _IN(0, 0.3, 0), _IN(0, 0.49, 0.66),
             _IN(0.7, 0.705, 0)],
  "capsule": _PAIR, "ellipsoid": _PAIR, "cylinder": _PAIR, "box": _BOX, "terrain_box": _BOX}


@functools.lru_cache(maxsize=None)
def model(kind):
  bodies = [P._free("c", "ellipsoid", SIZES[0]), P._free("d", "ellipsoid", SIZES[1])]
  ent = P.EntitySpec("pair", P._mjcf(bodies + ([P._free("p", *PARTNER[kind])] if kind in PARTNER else [])))
  if kind == "terrain_box":
    box = P.BoxSpec("terrain_0", pos=tuple(P.ST_POS), size=tuple(P.ST_SIZE))
    return P.compile_scene([ent], terrain="generator", terrain_geoms=[box], timestep=0.005)
  return P.compile_scene([ent], terrain="plane" if kind == "plane" else "none", timestep=0.005)


def pair_of(m, w):
  """World w's (probe ellipsoid, partner) geom ids."""
  ell = [g for g in range(m.ngeom) if int(m.geom_type[g]) == ELLIPSOID][:2]
  return ell[w % 2], [g for g in range(m.ngeom) if g not in ell][0]


@functools.lru_cache(maxsize=None)
def poses(kind):
  """(NW, nq) qpos, fp32-representable.  World w uses ellipsoid w % 2."""
  m, rng = model(kind), np.random.default_rng(KINDS.index(kind) + 41)
  q = np.zeros((NW, 21 if kind in PARTNER else 14))
  for w in range(NW):
    (k, i), s = (w % 2, w // 2), np.array(SIZES[w % 2])
    made = i < len(CONSTRUCTED[kind])
    q[w, 3::7] = 1.0
    q[w, 7 * (1 - k):7 * (1 - k) + 3] = 3.0  # parked
    fp, fq = (P.ST_POS, I) if kind == "terrain_box" else (np.zeros(3), I)
    if kind in PARTNER:
      fp, fq = (fp, fq) if made else (P.FX_POS, P.FX_QUAT)
      q[w, 14:17], q[w, 17:21] = fp, fq
    if made:
      qc, p0, gap = CONSTRUCTED[kind][i]
      if p0 == "edge":  # the lowest point over the box edge
        bs = P.ST_SIZE if kind == "terrain_box" else PARTNER["box"][1]
        p0 = np.array([bs[0] - E.support(R.Shape(ELLIPSOID, s, np.zeros(3), R.quat_mat(Y45)), (0, 0, -1))[0], 0.01, 0.5])
      else:
        p0 = np.array(p0[0]) * s + p0[1]
    else:
      qc, u = rng.normal(size=4), rng.normal(size=3)
      u = np.array([0.3 * u[0], 0.3 * u[1], 1.0]) if kind == "plane" else u
      p0 = 0.8 * u / np.linalg.norm(u)
      gap = (MARGIN + rng.uniform(0.002, 0.03), rng.uniform(0.1, 0.9) * MARGIN, -rng.uniform(0.02, 0.1) * s.min())[i % 3]
    q[w, 7 * k:7 * k + 3] = fp + R.quat_mat(fq) @ p0
    q[w, 7 * k + 3:7 * k + 7] = R.quat_mul(fq, qc / np.linalg.norm(qc))
    q[w] = q[w].astype(np.float32)
    if gap is not None:
      sh, (probe, part) = P.shapes(m, q[w]), pair_of(m, w)
      d, _, _, n = E.closest(sh[part], sh[probe])
      q[w, 7 * k:7 * k + 3] = (q[w, 7 * k:7 * k + 3] - n * (d - gap)).astype(np.float32)
  return q


def exact(A, B):
  """(signed distance, whether exact, direction).  Overlapping: closed form for the plane and the
  sphere (the ellipsoid's own signed distance of the centre), convex pairs minus the minimal depth."""
  d, _, _, n = E.closest(A, B)
  if d > TOUCH:
    return d, True, n
  if A.kind == PLANE:
    return -E.directional_depth(A, B, A.R[:, 2]), True, None
  if A.kind == SPHERE:
    return E.signed_distance(B, A.pos) - A.size[0], True, None
  return -E.minimal_depth(A, B)[0], False, None


@functools.lru_cache(maxsize=None)
def references(kind):
  """Per world (A, B, pair, exact(A, B), class), with the pose shares checked: reference only."""
  m, q, out = model(kind), poses(kind), []
  for w in range(NW):
    sh, (probe, part) = P.shapes(m, q[w]), pair_of(m, w)
    pair = (part, probe) if sh[part].kind < ELLIPSOID else (probe, part)  # by type, then by id
    ex = exact(sh[pair[0]], sh[pair[1]])
    cls = ("band" if abs(ex[0] - MARGIN) <= R.MARGIN_BAND else "out" if ex[0] > MARGIN else "near" if ex[0] > 0
           else "pen" if ex[0] >= -0.1 * min(SIZES[w % 2]) - 1e-7 else "deep")
    out.append((sh[pair[0]], sh[pair[1]], pair, ex, cls))
  share = collections.Counter(o[4] for o in out)
  assert share["band"] <= 0.05 * NW and min(share["out"], share["near"], share["pen"]) >= NW // 4, share
  return out


def check(kind, eng):
  dtol, stol, ntol = ((D_TOL + CONVEX_DIST, D_TOL + CONVEX_SURF, N_TOL + CONVEX_N) if kind in CONVEX else
                      (D_TOL + SPHERE_TOL, D_TOL + SPHERE_TOL, N_TOL + SPHERE_N) if kind == "sphere" else (D_TOL, D_TOL, N_TOL))
  worst, fails = collections.Counter(), []
  for w, (A, B, pair, (sd, ex, n), cls) in enumerate(references(kind)):
    cons = eng[w]
    try:
      assert cls != "out" or len(cons) == 0, f"{len(cons)} contacts at exact distance {sd:.6g} > margin"
      if cls in ("band", "out"):
        continue
      assert len(cons) == 1 and np.array_equal(cons[0, :2], pair), f"{len(cons)} contacts, geoms {cons[:, :2].tolist()}"
      dist, pos, nn = cons[0, 2], cons[0, 3:6], cons[0, 6:9]
      assert abs(np.linalg.norm(nn) - 1) <= N_TOL and dist <= MARGIN + D_TOL, f"|n|, dist {dist}"
      for S, pt in ((A, pos - nn * dist / 2), (B, pos + nn * dist / 2)):
        worst["surf"] = max(worst["surf"], abs(E.signed_distance(S, pt)))
        assert abs(E.signed_distance(S, pt)) <= stol, f"surface point off geom kind {S.kind} by {abs(E.signed_distance(S, pt)):.3g}"
      ref = sd if ex else -E.directional_depth(A, B, nn)  # (convex, overlapping: the depth along n)
      worst["dist"], worst["ratio"] = max(worst["dist"], abs(dist - ref)), max(worst["ratio"], 0.0 if ex else dist / sd)
      assert abs(dist - ref) <= dtol, f"dist {dist:.9g} vs {ref:.9g}"
      if n is not None and sd + A.radius > 4 * EPS32:
        worst["normal"] = max(worst["normal"], np.abs(nn - n).max())
        assert np.abs(nn - n).max() <= ntol, f"normal off by {np.abs(nn - n).max():.3g}"
    except AssertionError as exn:
      fails.append(f"world {w}: {exn}")
  print(f"\n[ellipsoid {kind}] maxima: " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
  assert not fails and worst["ratio"] <= 1.5 * DEPTH_RATIO_MEASURED, f"{kind}: {len(fails)} failures\n" + "\n".join(fails[:12])


@pytest.mark.parametrize("kind", KINDS)
def test_ellipsoid_pair_against_exact_geometry(kind, gpu_device):
  import test_gpu_narrowphase_pairs as G
  references(kind)  # the pose shares, before anything runs on the GPU
  # (engine_contacts asserts unsupported == 0, which an engine without ellipsoids fails, and con_overflow == 0)
  check(kind, G.engine_contacts(types.SimpleNamespace(model=model(kind)), poses(kind).astype(np.float32), gpu_device))


def test_ellipsoid_rests_like_a_sphere(gpu_device):
  """One step() of an oblate ellipsoid (a, a, c) on the plane beside a sphere of radius c, same inertial."""
  from mjlab_amd import jit
  from mjlab_amd.sim import MujocoCfg, Simulation, SimulationCfg
  c = 0.04
  ent = P.EntitySpec("pair", P._mjcf([P._free("e", "ellipsoid", (0.1, 0.1, c)), P._free("s", "sphere", (c,))]))
  m = P.compile_scene([ent], terrain="plane", timestep=0.005)
  assert "ellipsoid" in jit.ineligible(m)
  mk = lambda sp: SimulationCfg(nconmax=16, njmax=64, specialize=sp, mujoco=MujocoCfg(timestep=0.005, iterations=20, ls_iterations=20))
  with pytest.raises(NotImplementedError, match="ellipsoid"):
    Simulation(4, mk("always"), m, gpu_device)
  sim = Simulation(4, mk("never"), m, gpu_device)
  d, q = sim.data, np.zeros((4, 14), np.float32)
  q[:, 3::7], q[:, 2::7], q[:, 7] = 1.0, c - 0.001, 1.0
  d.qpos[:] = torch.as_tensor(q)
  d.qvel.zero_()
  d.qacc_warmstart.zero_()
  sim.step()
  torch.cuda.synchronize()
  st, ncon = sim.stats(), d.ncon.cpu().numpy().reshape(4)
  assert sim.info()["spec"] == 0 and np.array_equal(ncon, [2] * 4), (sim.info(), ncon)
  assert torch.isfinite(d.qacc).all() and st["unsupported"] == 0 and st["con_overflow"] == 0, st
  geom = d.contact_geom.reshape(4, -1, 2).cpu().numpy()
  fn, gt = d.contact_force.reshape(4, -1, 3).cpu().numpy()[..., 0], np.asarray(m.geom_type)
  for w in range(4):
    f = {t: fn[w, :2][gt[geom[w, :2, 1]] == t].sum() for t in (ELLIPSOID, SPHERE)}
    print(f"[ellipsoid step] world {w}: normal force ellipsoid {f[ELLIPSOID]:.6g} sphere {f[SPHERE]:.6g} m g 9.81")
    assert abs(f[ELLIPSOID] - f[SPHERE]) <= 2 * abs(f[SPHERE] - 9.81), f
