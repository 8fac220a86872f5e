"""Every narrowphase pair on the GPU: the engine's contacts against the oracle's, contact by
contact, and against the exact geometry of narrowphase_ref directly.

The scenes and their 64 poses are test_narrowphase_pairs.py's (one Simulation per scene, one
world per pose, `forward()` only); both sides take the poses rounded to fp32.  Between them
the scenes reach every dispatch branch of both collision loops: plane / sphere / capsule /
box pairs of the regular loop (dynamic box against dynamic box included), hfield and static
box blocks of the terrain loop (an axis-aligned terrain box, a box turned about a skew axis
with its geom index below and above the probe's), all three `box_box` kinds and an
8-point `box_face_clip` -- asserted from the contacts (test_narrowphase_pairs.expectations).

Engine against oracle: ncon, contact_geom and the order equal; dist and pos within 2e-6,
the normal within 2e-5 (what test_gpu_capsule_capsule.py holds at these sizes).  The copies
translated by (80, -60, 0) add the rounding of the inputs, 4 eps32 (max |coordinate| + r1 +
r2), to dist and pos, and that over the core distance to a normal that is a normalised
difference of points (sphere-swept pairs, hfield).  A normal whose core distance is below
that rounding (a sphere centre placed on a box's face, edge or corner, on a capsule's axis
or on another sphere's centre) is undefined in fp32, and with it the point r + dist / 2
along it: there dist alone is compared.

Capsule-box contacts at an interior point of the segment: an fp32 golden-section search
resolves the minimiser of a function flat to second order only to about sqrt(eps32) of the
segment, so their pos bound is measured, not derived: engine minus oracle over these seeds
is at most 1.36e-5 (see CAPSULE_MID_POS below), the bound 4 x that, capped at kBoxMidEps =
1e-4; their normal turns by that over the core distance.

Engine against the exact geometry: statements (a) and (b) with the same bounds plus the
oracle-to-reference tolerances.  hfield contacts of a sphere centre below the surface (the
build's own `sd < 0` rule) are compared with the oracle only.
"""

import numpy as np
import pytest
import torch

import narrowphase_ref as R
import test_narrowphase_pairs as P
from narrowphase_ref import BOX, CAPSULE, HFIELD, PLANE, SPHERE

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
D_TOL, N_TOL = 2e-6, 2e-5
# largest |pos engine - pos oracle| of a capsule-box interior contact over the committed seeds
# (capsule_box, static_capsule, turned_capsule; measured on an MI355X), and the bound from it
CAPSULE_MID_POS_MEASURED = 1.36e-5
CAPSULE_MID_POS = min(4 * CAPSULE_MID_POS_MEASURED, R.BOX_MID_EPS)


def engine_contacts(sc, q32, device):
  from mjlab_amd.sim import MujocoCfg, Simulation, SimulationCfg
  m, n = sc.model, len(q32)
  cfg = SimulationCfg(nconmax=P.NCONMAX, njmax=4 * P.NCONMAX,
                      mujoco=MujocoCfg(timestep=m.timestep, iterations=10, ls_iterations=20))
  sim = Simulation(n, cfg, m, device)
  d = sim.data
  d.qpos[:] = torch.as_tensor(q32)
  d.qvel.zero_()
  d.qacc_warmstart.zero_()
  sim.forward()
  torch.cuda.synchronize()
  st = sim.stats()
  assert st["unsupported"] == 0 and st["con_overflow"] == 0, st
  ncon = d.ncon.cpu().numpy().reshape(n)
  geom = d.contact_geom.reshape(n, -1, 2).cpu().numpy()
  dist = d.contact_dist.reshape(n, -1).cpu().numpy()
  pos = d.contact_pos.reshape(n, -1, 3).cpu().numpy()
  frame = d.contact_frame.reshape(n, -1, 9).cpu().numpy()
  out = []
  for w in range(n):
    k = int(ncon[w])
    out.append(np.concatenate([geom[w, :k], dist[w, :k, None], pos[w, :k], frame[w, :k, :3]],
                              axis=1).astype(np.float64))
  return out


def _is_mid(A, con):
  """A capsule-box contact (capsule geom 1) whose sphere sits inside the segment."""
  c = con[3:6] - con[6:9] * (con[2] / 2 + A.radius)
  return abs(float((c - A.pos) @ A.R[:, 2])) < A.size[1] - 1e-6


@pytest.mark.parametrize("name", P.SCENES)
def test_engine_pair_against_oracle_and_exact_geometry(name, gpu_device):
  sc = P.scene(name)
  m = sc.model
  q32 = sc.q.astype(np.float32)
  q = q32.astype(np.float64)
  eng = engine_contacts(sc, q32, gpu_device)
  import oracle_lib as ol
  ora = []
  for w in range(len(q)):
    f = ol.forward(m, q[w], nconmax=P.NCONMAX, njmax=4 * P.NCONMAX)
    assert f["overflow"] == 0
    ora.append(f["contact"])
  rb = np.asarray(m.geom_rbound, float)
  worst = dict(dist=0.0, pos=0.0, normal=0.0, mid_pos=0.0)
  fails, stats = [], []
  for w in range(len(q)):
    e, o = eng[w], ora[w]
    if len(e) != len(o) or not np.array_equal(e[:, :2], o[:, :2]):
      fails.append(f"world {w}: engine geoms {e[:, :2].tolist()} vs oracle {o[:, :2].tolist()}")
      stats.append(dict(out=False, con=len(o) > 0, below=False, kinds=set()))
      continue
    sh = P.shapes(m, q[w])
    far = w >= P.NPOSE
    extra_w = 0.0
    for i in range(len(o)):
      A, B = sh[int(o[i, 0])], sh[int(o[i, 1])]
      coord = max(np.abs(A.pos).max() if A.kind != PLANE else 0.0, np.abs(B.pos).max())
      extra = 4 * EPS32 * (coord + rb[int(o[i, 0])] + rb[int(o[i, 1])])
      extra_w = max(extra_w, extra if far else 0.0)
      dtol = D_TOL + (extra if far else 0.0)
      ptol, ntol = dtol, N_TOL
      # normals that are normalised point differences: the inputs' rounding over the distance
      c = R.closest(A, B)
      if A.kind in (SPHERE, CAPSULE, HFIELD):
        if abs(c.core) <= extra:  # the point sits r + dist / 2 along the normal: undefined with it
          ntol = ptol = np.inf
        elif far:
          ntol += extra / abs(c.core)
      mid = (A.kind, B.kind) == (CAPSULE, BOX) and _is_mid(A, o[i])
      dpos = e[i, 3:6] - o[i, 3:6]
      if mid and not c.unique:
        # the segment runs along a face or an edge: every point of the stretch is a minimiser
        # and the two searches stop at different ones; compared across the axis only
        dpos = dpos - A.R[:, 2] * float(dpos @ A.R[:, 2])
      elif mid and np.isfinite(ptol):
        worst["mid_pos"] = max(worst["mid_pos"], np.abs(dpos).max())
        ptol += CAPSULE_MID_POS
        ntol += CAPSULE_MID_POS / max(abs(c.core), 1e-300)
      elif np.isfinite(ptol):
        worst["pos"] = max(worst["pos"], np.abs(e[i, 3:6] - o[i, 3:6]).max() - (extra if far else 0.0))
      err = (abs(e[i, 2] - o[i, 2]), np.abs(dpos).max(), np.abs(e[i, 6:9] - o[i, 6:9]).max())
      worst["dist"] = max(worst["dist"], err[0] - (extra if far else 0.0))
      if np.isfinite(ntol) and not mid:
        worst["normal"] = max(worst["normal"], err[2] - (ntol - N_TOL))
      if err[0] > dtol or err[1] > ptol or err[2] > ntol:
        fails.append(f"world {w} contact {i}: dist/pos/normal off by {err[0]:.3g} {err[1]:.3g} "
                     f"{err[2]:.3g} (bounds {dtol:.3g} {ptol:.3g} {ntol:.3g})")
    # the engine against the exact geometry
    tol = P.Tol(d=D_TOL + extra_w + 1e-9, n=N_TOL + 1e-9, golden=D_TOL + extra_w + 1e-8,
                inside=D_TOL + extra_w + 1e-5, mid_pos=CAPSULE_MID_POS,
                core_eps=4 * EPS32 * (np.abs(q[w, :3]).max() + 0.5))
    try:
      stats.append(P.check_world(m, q[w], e, tol))
    except AssertionError as ex:
      fails.append(f"world {w} against exact geometry: {ex}")
      stats.append(dict(out=False, con=len(e) > 0, below=False, kinds=set()))
  print(f"\n[narrowphase {name}] engine - oracle maxima beyond the inputs' rounding: "
        + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
  assert not fails, f"{name}: {len(fails)} failures\n" + "\n".join(fails[:12])
  assert worst["mid_pos"] <= CAPSULE_MID_POS  # a larger difference is a finding, not a tolerance
  P.check_caps(sc, stats)
  # (fp32 poses: the sphere sits exactly on the other sphere's centre, only near a capsule's axis)
  P.expectations(sc, [len(c) for c in eng], stats,
                 [c[0, 6:9] if len(c) else None for c in eng] if name == "sphere_sphere" else None)
