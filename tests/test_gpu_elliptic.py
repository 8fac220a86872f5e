"""The engine's elliptic friction cones (`cone="elliptic"`: dim rows per contact, the cone-aware
Newton solver, the wrench decode) on the scenes of tests/elliptic_scenes.py against the
independent fp64 reference tests/elliptic_ref.py.  The oracle never learns about cones: these
scenes are held to the reference only, which takes one engine output, the contact frame's
tangents, after checking the frame (constraint_ref.check_frame).

Seven single-contact scenes, the 24-contact `plate`, `overflow` (the plate from a fast carve it
exceeds, re-solved at max capacity) and `mixed`, each at 32, 1 and 70 worlds on the generic kernels
(`specialize="never"`), one forward() and one step() per scene and batch, one GPU child process
for the whole module (tests/elliptic_child.py).  Every world has its own expanded geom_friction, geom_solref,
geom_solimp and geom_margin.  `mixed` puts a joint-equality pair, a limited slide at its limit, a
condim-1 contact and an elliptic contact in one world (five single-dof bodies, M analytic): the
ordinary rows of the cone solver; every scene also runs at 1 and 70 worlds.

Per world:
  ncon nefc contact_geom  equal (dim rows per contact; tie clearance 2e-4); no world is left out
  contact_dist            atol 2e-5
  qacc                    B_a = 2e-3 max(1, max|qacc|)   (test_gpu_parity's bound)
  qvel / qpos             h x / h^2 x the qacc bound + 1e-5
  row force f_i           e_i = sum_k S_ik (|J| B_a)_k + c eps32 sum_k S_ik (|aref| + |J| |a|)_k with
                          S = |H_c| in the middle zone, diag(D) otherwise (elliptic_ref.force_bounds)
  qfrc_constraint_j       sum_i |J_ij| e_i
  contact_force / torque  e of rows 0-2 / 3-5
  wrench consistency      qfrc_constraint = J' (decoded wrench) with the reference's rows J, within
                          c eps32 sum_i Jmag_ij |f_i| (+ 1e-6 of the largest; Jmag: the magnitudes
                          of the terms an fp32 row entry sums, which exceed |J| where a lever arm
                          cancels): phase B's J' f against phase C's decode
  middle zone             | |f_t / friction| - f_0 | <= c eps32 f_0 from the engine's own outputs
  slider                  the world-frame tangential force is antiparallel to the sliding velocity
                          (its component across the velocity within the tangential force bound):
                          the check a pyramidal build cannot pass
c = FORCE_C = 32 (tests/test_gpu_constraint_params.py).  Measured multiples of eps32, largest
err / bound per scene and Newton iterations on an MI355X: MEASURED below (the largest ratios over
all scenes: qacc 0.012, qvel 0.021, forces 0.072, wrench 0.30, cone 0.055; 2 to 7 iterations).
The child's run time: 4.2 s; its time limit is ten times that.

Step paths: step(4), four step(1) and a replayed graph of step(4) are bit-identical in
parity_util.DATA_FIELDS and contact_torque (mixed, 1 and 70 worlds).  Expanded fields at
the model's values: bit-identical.  Contact sensor: the `force` and `torque` slots equal the
decoded wrench.  Rollout: 200 steps of the puck sliding 30 degrees off the frame's tangent.  The
cone's normal force answers the sliding speed (aref_t = -B v_t), so the onset of sliding lifts the
puck and the per-step fall of the speed is not f0 g h; what holds exactly is the momentum
identity speed_0 - speed_k = f0 (g k h + vz_k - vz_0) while it slides, asserted within the
accumulated per-step qvel bounds, as are the lateral drift (the reference rollout's own plus 200
per-step qpos bounds) and rest at the end.

A child that is killed at its time limit, exits with 134 / 139 / a negative status or reports a
HIP illegal access sets a module flag; every later test fails without starting anything.
"""

from __future__ import annotations

import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import elliptic_ref as ref
import elliptic_scenes as sc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# the child took 4.2 s on an MI355X (37 sims; most of it start-up and the sims' creation); ten times that
CHILD_SECONDS = 4.2
CHILD_TIMEOUT = int(10 * CHILD_SECONDS)
EPS32 = float(np.finfo(np.float32).eps)
FORCE_C = 32.0
NS = (sc.NWORLD, 1, 70)  # 1: the single-world launch; 70: past one wave of worlds, worlds repeat
BATCHES = {name: list(NS) for name in sc.SCENES + ("plate", "mixed")}
PATHS_SCENE = "mixed"
SENSOR_SCENE = "ball_tilted6"
# Floor of a dof's wrench-consistency bound, as a fraction of the largest dof's: the floor
# tests/test_gpu_condim.py puts under the same comparison (its many70 scene), for dofs whose own
# terms vanish while their fp32 sum collects the other dofs' rounding through the rows
WRENCH_FLOOR = 1e-6
# per scene on an MI355X, 32 worlds (70 worlds: the same figures; 1 world: smaller): measured
# multiple of eps32 of the force errors, largest err / bound of qacc, qvel, the forces (qfrc,
# contact force and torque), the wrench consistency and the cone equality, and the Newton
# iterations (max over worlds).  DESIGN.md section 9 holds the same table.
MEASURED = {
  "slider":          dict(c=0.8, qacc=0.000, qvel=0.001, force=0.000, wrench=0.000, cone=0.030, niter=2),
  "slider_impratio": dict(c=0.9, qacc=0.000, qvel=0.002, force=0.000, wrench=0.000, cone=0.044, niter=2),
  "ball_tilted3":    dict(c=19.2, qacc=0.012, qvel=0.012, force=0.000, wrench=0.094, cone=0.026, niter=3),
  "ball_tilted4":    dict(c=19.2, qacc=0.012, qvel=0.020, force=0.056, wrench=0.087, cone=0.027, niter=5),
  "ball_tilted6":    dict(c=1560.9, qacc=0.008, qvel=0.021, force=0.072, wrench=0.076, cone=0.036, niter=6),
  "two_balls":       dict(c=9.1, qacc=0.002, qvel=0.004, force=0.001, wrench=0.299, cone=0.033, niter=5),
  "pad_hinge":       dict(c=24.7, qacc=0.002, qvel=0.005, force=0.003, wrench=0.027, cone=0.028, niter=3),
  "plate":           dict(c=3.8, qacc=0.004, qvel=0.004, force=0.000, wrench=0.131, cone=0.055, niter=7),
  "overflow":        dict(c=3.8, qacc=0.004, qvel=0.004, force=0.000, wrench=0.131, cone=0.055, niter=7),
  "mixed":           dict(c=13.9, qacc=0.003, qvel=0.006, force=0.000, wrench=None, cone=0.040, niter=3),
}
# (ball_tilted6's multiple of eps32, 1560.9, is in the worlds whose torsional and rolling
# coefficients sit at MINMU: D_j = D_1 f0^2 / MINMU^2 there, and the bound's first term, the
# force's sensitivity times the qacc bound, covers it at 0.072; FORCE_C = 32 stands.)

_faulted = []


def _run_child(tmp):
  if _faulted:
    pytest.fail(f"not run: an earlier child faulted ({_faulted[0]})")
  job, out = os.path.join(tmp, "job.json"), os.path.join(tmp, "out")
  os.makedirs(out, exist_ok=True)
  with open(job, "w") as fh:
    json.dump({"scenes": list(sc.SCENES) + ["plate", "mixed"], "batches": BATCHES, "overflow": list(NS),
               "paths": [PATHS_SCENE, [1, 70]],
               "sensor": SENSOR_SCENE, "same": SENSOR_SCENE, "rollout": True}, fh)
  cmd = [sys.executable, os.path.join(HERE, "elliptic_child.py"), job, out]
  t0 = time.perf_counter()
  try:
    r = subprocess.run(cmd, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
  except subprocess.TimeoutExpired as e:
    done = (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
    _faulted.append(f"killed at its {CHILD_TIMEOUT} s limit after: {done[-200:]}")
    pytest.fail(f"child hung: {_faulted[0]}")
  print(f"elliptic child took {time.perf_counter() - t0:.1f} s")
  text = (r.stdout or "") + (r.stderr or "")
  if r.returncode in (134, 139) or r.returncode < 0 or "illegal memory access" in text:
    _faulted.append(f"exit status {r.returncode} after: {(r.stdout or '')[-200:]}")
    pytest.fail(f"child faulted ({r.returncode}):\n{text[-3000:]}")
  assert r.returncode == 0, f"child failed ({r.returncode}):\n{text[-3000:]}"
  res = {}
  for f in sorted(os.listdir(out)):
    if f.endswith(".npz") and not f.startswith("."):
      with np.load(os.path.join(out, f)) as z:
        res[f[:-4]] = {k: z[k] for k in z.files}
  return res


@pytest.fixture(scope="module")
def ran(gpu_device, tmp_path_factory):
  return _run_child(str(tmp_path_factory.mktemp("elliptic")))


def _ratio(err, bound):
  err, bound = np.abs(np.asarray(err, float)), np.asarray(bound, float)
  if not err.size:
    return 0.0
  return float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-300))))


def _world(out, w):
  return {k[5:]: v[w] for k, v in out.items() if k.startswith("step_")}


def check_scene(name, out, n):
  h = sc.H
  m = sc.model(name)
  gid = {g: i for i, g in enumerate(m.names["geom"])}
  R = dict(dist=0.0, qacc=0.0, qvel=0.0, qpos=0.0, qfrc=0.0, cforce=0.0, ctorque=0.0, wrench=0.0, cone=0.0, across=0.0)
  cmeas, bad, nrows, zones, niter = 0.0, [], set(), set(), 0

  def expect(ok, msg):
    if not ok:
      bad.append(msg)

  for wi in range(n):
    w = wi % sc.NWORLD
    t = _world(out, wi)
    ncon, nefc = int(t["ncon"].reshape(-1)[0]), int(t["nefc"].reshape(-1)[0])
    frame = t["contact_frame"].reshape(-1, 9)[0].astype(float) if ncon else None
    r = sc.reference(name, w, frame=frame)
    fw = (int(out["fwd_ncon"][wi].reshape(-1)[0]), int(out["fwd_nefc"][wi].reshape(-1)[0]))
    expect(fw == (r["ncon"], r["nefc"]), f"world {wi}: forward ncon / nefc {fw} vs {r['ncon']} / {r['nefc']}")
    same = (ncon, nefc) == (r["ncon"], r["nefc"])
    expect(same, f"world {wi}: step ncon / nefc {ncon} / {nefc} vs {r['ncon']} / {r['nefc']}")
    if not same:
      continue
    nrows.add(nefc)
    zones.update(r["contact_zone"])
    niter = max(niter, int(t["solver_niter"].reshape(-1)[0]))
    _, g1, g2 = sc.world_geometry(name, w, *(x[w] for x in sc.states(name)))[:3]
    if ncon:
      expect(tuple(int(x) for x in t["contact_geom"].reshape(-1, 2)[0]) == (gid[g1], gid[g2]), f"world {wi}: contact_geom")
      for dk in (t["contact_dist"].reshape(-1)[0], out["fwd_contact_dist"][wi].reshape(-1)[0]):
        c = _ratio(dk - r["dist"], 2e-5)
        expect(c <= 1.0, f"world {wi}: contact_dist {c:.2f} x 2e-5")
        R["dist"] = max(R["dist"], c)
    ab = np.full(r["qacc"].size, 2e-3 * max(1.0, float(np.abs(r["qacc"]).max())))
    c = _ratio(out["fwd_qacc"][wi] - r["qacc"], ab)
    expect(c <= 1.0, f"world {wi}: forward qacc {c:.2f} of its bound")
    for key, got, bound in (("qacc", t["qacc"], ab), ("qvel", t["qvel"], ab * h + 1e-5),
                            ("qpos", t["qpos"], ab.max() * h * h + 1e-5)):
      c = _ratio(got - r[key], bound)
      expect(c <= 1.0, f"world {wi}: {key} {c:.2f} of its bound (zones {r['contact_zone']})")
      R[key] = max(R[key], c)
    first, mag = ref.force_bounds(r, ab)
    J = r["Jmag"]
    dim = r["dim"] if nefc else 0
    cf = t["contact_force"].reshape(-1, 3)[0].astype(float)
    ct = t["contact_torque"].reshape(-1, 3)[0].astype(float) if "contact_torque" in t else np.zeros(3)
    pad = lambda e: np.concatenate([e, np.zeros(6 - e.size)])
    wf, wm = pad(first), pad(mag)
    rf = r["contact_force"][0] if ncon else np.zeros(3)
    rt = r["contact_torque"][0] if ncon else np.zeros(3)
    errs = [(t["qfrc_constraint"] - r["qfrc_constraint"], J.T @ first if nefc else np.zeros(J.shape[1]),
             J.T @ mag if nefc else np.zeros(J.shape[1]), "qfrc"),
            (cf - rf, wf[:3], wm[:3], "cforce"), (ct - rt, wf[3:], wm[3:], "ctorque")]
    for err, b_first, b_mag, key in errs:
      cmeas = max(cmeas, _ratio(err, EPS32 * b_mag) if np.any(b_mag > 0) else 0.0)
      expect(np.all(np.abs(err)[b_mag == 0] == 0.0), f"world {wi}: {key} {err} without an active row")
      c = _ratio(err, b_first + FORCE_C * EPS32 * b_mag)
      expect(c <= 1.0, f"world {wi}: {key} {c:.2f} of its bound")
      R[key] = max(R[key], c)
    expect(not np.any(t["contact_force"].reshape(-1, 3)[1:]), f"world {wi}: force past the contact")
    if not nefc:
      continue
    # wrench consistency: phase B's J' f against phase C's decode through the reference's rows
    fe = np.concatenate([cf, ct])[:dim]
    want = r["J"].T @ fe
    wb = FORCE_C * EPS32 * (r["Jmag"].T @ np.abs(fe))
    wb = np.maximum(wb, WRENCH_FLOOR * wb.max())
    c = _ratio(t["qfrc_constraint"].astype(float) - want, wb)
    expect(c <= 1.0, f"world {wi}: qfrc_constraint vs J' wrench {c:.2f} of its bound")
    R["wrench"] = max(R["wrench"], c)
    if r["contact_zone"] == [ref.MIDDLE]:
      fr = r["fr"][:dim - 1]
      c = _ratio(np.linalg.norm(fe[1:] / fr) - fe[0], FORCE_C * EPS32 * fe[0])
      expect(c <= 1.0, f"world {wi}: |f_t / friction| = {np.linalg.norm(fe[1:] / fr)} vs f_0 = {fe[0]}")
      R["cone"] = max(R["cone"], c)
      if name.startswith("slider"):
        F = r["frame"]
        v = sc.states(name)[1][w]
        vt = v - F[0] * (F[0] @ v)
        ftw = F[1] * fe[1] + F[2] * fe[2]
        vh = vt / np.linalg.norm(vt)
        across = ftw - vh * (vh @ ftw)
        tb = float(np.linalg.norm((first + FORCE_C * EPS32 * mag)[1:3]))
        c = _ratio(np.linalg.norm(across), tb)
        expect(vh @ ftw < 0 and c <= 1.0, f"world {wi}: tangential force {ftw} is not antiparallel to {vt}")
        R["across"] = max(R["across"], c)
  print(f"{name} x {n}: nefc {sorted(nrows)} zones {sorted(zones)} niter {niter} measured c {cmeas:.1f} ratios "
        + " ".join(f"{k} {v:.3f}" for k, v in R.items()))
  assert not bad, f"{name} x {n}: {len(bad)} mismatches, first: " + "; ".join(bad[:6])
  assert nrows == {0, sc.DIM[name]} or n == 1
  if name.startswith("slider") and n >= sc.NWORLD:
    assert zones == {ref.TOP, ref.BOTTOM, ref.MIDDLE}
  return R, cmeas


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", sc.SCENES)
def test_engine_matches_the_reference(name, n, ran):
  out = ran[f"{name}_{n}"]
  assert out["info"][0] == 0 and out["info"][1] == 0, "specialize='never' ran a specialised kernel"
  st = dict(zip(("max_ncon", "max_nefc", "con_overflow", "row_overflow", "unsupported", "resolved"), out["stats"]))
  assert st["unsupported"] == 0 and st["con_overflow"] == 0 and st["row_overflow"] == 0, st
  assert st["max_nefc"] == (sc.DIM[name] if n > 1 else st["max_nefc"]), st
  check_scene(name, out, n)


def check_multi(name, out, n):
  """`plate` / `overflow` / `mixed`: several contacts and (mixed) ordinary rows in one world.  The
  engine's contact order (contact_geom) and frames go to the reference; every world is compared."""
  h = sc.H
  scene = "plate" if name == "overflow" else name
  names = sc.model(scene).names["geom"]
  nv = sc.states(scene)[1].shape[1]
  R = dict(qacc=0.0, qvel=0.0, qpos=0.0, qfrc=0.0, cforce=0.0, wrench=0.0, cone=0.0)
  zones, niter, cmeas, bad, rows = set(), 0, 0.0, [], set()
  for wi in range(n):
    w = wi % sc.NWORLD
    t = _world(out, wi)
    ncon, nefc = int(t["ncon"].reshape(-1)[0]), int(t["nefc"].reshape(-1)[0])
    geoms = t["contact_geom"].reshape(-1, 2)[:ncon]
    frames = t["contact_frame"].reshape(-1, 9)[:ncon].astype(float)
    moving = [names[g1] if names[g1] != "floor" else names[g2] for g1, g2 in geoms]
    assert all("floor" in (names[g1], names[g2]) for g1, g2 in geoms), f"world {wi}: contact_geom {geoms}"
    if scene == "plate":
      assert sorted(moving) == sorted(f"s{k}" for k in range(sc.PLATE_NCON)), f"world {wi}: contact_geom {geoms}"
      r = sc.plate_reference(w, [int(g[1:]) for g in moving], frames)
    else:
      r = sc.mixed_reference(w, moving, frames)
    assert (ncon, nefc) == (r["ncon"], r["nefc"]), f"world {wi}: {ncon} / {nefc} vs the reference's {r['ncon']} / {r['nefc']}"
    assert (int(out["fwd_ncon"][wi].reshape(-1)[0]), int(out["fwd_nefc"][wi].reshape(-1)[0])) == (ncon, nefc)
    rows.add(nefc)
    zones.update(r["contact_zone"])
    niter = max(niter, int(t["solver_niter"].reshape(-1)[0]))
    ab = np.full(nv, 2e-3 * max(1.0, float(np.abs(r["qacc"]).max())))
    for key, got, bound in (("qacc", out["fwd_qacc"][wi], ab), ("qacc", t["qacc"], ab), ("qvel", t["qvel"], ab * h + 1e-5),
                            ("qpos", t["qpos"], ab.max() * h * h + 1e-5)):
      c = _ratio(got - r[key], bound)
      if c > 1.0:
        bad.append(f"world {wi}: {key} {c:.2f} of its bound")
      R[key] = max(R[key], c)
    first, mag = ref.force_bounds(r, ab)
    cf = t["contact_force"].reshape(-1, 3)[:ncon].astype(float)
    # the contacts' rows behind the ordinary ones, dim rows each (a contact without rows: none)
    k0 = sum(g["D"].size for g in r["groups"][:r.get("nextra", 0)])
    fe, fr_ref = [], []
    for k, c in enumerate(r["contacts"]):
      d = c["dim"] if c["group"] is not None else 0
      fe.append(cf[k, :d])
      fr_ref.append(r["contact_force"][k][:d])
      assert not np.any(cf[k, d:]), f"world {wi} contact {k}: force past its dimension"
    fe, fr_ref = np.concatenate(fe) if fe else np.zeros(0), np.concatenate(fr_ref) if fr_ref else np.zeros(0)
    for err, b_first, b_mag, key in ((t["qfrc_constraint"] - r["qfrc_constraint"], r["Jmag"].T @ first, r["Jmag"].T @ mag, "qfrc"),
                                     (fe - fr_ref, first[k0:], mag[k0:], "cforce")):
      cmeas = max(cmeas, _ratio(err, EPS32 * b_mag))
      c = _ratio(err, b_first + FORCE_C * EPS32 * b_mag)
      if c > 1.0:
        bad.append(f"world {wi}: {key} {c:.2f} of its bound")
      R[key] = max(R[key], c)
    assert not np.any(t["contact_torque"]) and not np.any(t["contact_force"].reshape(-1, 3)[ncon:])
    if k0 == 0:  # (the ordinary rows' forces are no output: no wrench to rebuild qfrc_constraint from)
      wb = FORCE_C * EPS32 * (r["Jmag"].T @ np.abs(fe))
      c = _ratio(t["qfrc_constraint"].astype(float) - r["J"].T @ fe, np.maximum(wb, WRENCH_FLOOR * wb.max()))
      R["wrench"] = max(R["wrench"], c)
      if c > 1.0:
        bad.append(f"world {wi}: qfrc_constraint vs J' wrench {c:.2f} of its bound")
    for k, z in enumerate(r["contact_zone"]):
      if z == ref.MIDDLE:
        fr = r["contacts"][k]["fr"][:2]
        c = _ratio(np.linalg.norm(cf[k, 1:] / fr) - cf[k, 0], FORCE_C * EPS32 * cf[k, 0])
        R["cone"] = max(R["cone"], c)
        if c > 1.0:
          bad.append(f"world {wi} contact {k}: |f_t / friction| vs f_0 {c:.2f} of its bound")
  print(f"{name} x {n}: nefc {sorted(rows)} zones {sorted(zones)} niter {niter} measured c {cmeas:.1f} ratios "
        + " ".join(f"{k} {v:.3f}" for k, v in R.items()))
  assert not bad, f"{name} x {n}: {len(bad)} mismatches, first: " + "; ".join(bad[:6])
  return zones, rows


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ["plate", "overflow"])
def test_plate_matches_the_reference(name, n, ran):
  """24 contacts / 72 rows per world: rows past one per lane; `overflow`: the same worlds from a
  16-contact / 48-row fast carve, re-solved at max capacity (the multi-round contact loops)."""
  out = ran[f"{name}_{n}"]
  st = dict(zip(("max_ncon", "max_nefc", "con_overflow", "row_overflow", "unsupported", "resolved"), out["stats"]))
  assert out["info"][0] == 0 and out["info"][1] == 0
  assert st["unsupported"] == 0 and st["con_overflow"] == 0 and st["row_overflow"] == 0, st
  assert (st["max_ncon"], st["max_nefc"]) == (sc.PLATE_NCON, 3 * sc.PLATE_NCON), st
  assert (st["resolved"] >= n) == (name == "overflow"), st
  zones, rows = check_multi(name, out, n)
  assert rows == {3 * sc.PLATE_NCON}
  assert zones == {ref.TOP, ref.BOTTOM, ref.MIDDLE} or n == 1, zones


@pytest.mark.parametrize("n", NS)
def test_mixed_rows_in_one_problem(n, ran):
  """A joint-equality pair, a limit row, a condim-1 contact and an elliptic contact in one world:
  the ordinary rows' branches of the cone solver and their group word -1."""
  out = ran[f"mixed_{n}"]
  st = dict(zip(("max_ncon", "max_nefc", "con_overflow", "row_overflow", "unsupported", "resolved"), out["stats"]))
  assert out["info"][0] == 0 and out["info"][1] == 0
  assert st["unsupported"] == 0 and st["con_overflow"] == 0 and st["row_overflow"] == 0, st
  zones, rows = check_multi("mixed", out, n)
  if n > 1:
    assert 7 in rows and zones == {ref.TOP, ref.BOTTOM, ref.MIDDLE}, (rows, zones)


@pytest.mark.parametrize("n", [1, 70])
def test_step_paths_are_bit_identical(n, ran):
  out = ran[f"paths_{n}"]
  rep = json.loads(str(out["paths"]))
  for k in ("single", "graph"):
    assert not rep[k]["fields"], f"{n} worlds: step(4) differs from {k}: {rep[k]}"
  assert int(out["nefc_max"]) >= (7 if n > 1 else 3) and float(out["moved"]) > 1e-4


def test_expanded_fields_at_model_values_change_nothing(ran):
  rep = json.loads(str(ran["same"]["same"]))
  for what in ("fwd", "step"):
    assert not rep[what]["fields"], f"expanded fields at the model's values differ after {what}: {rep[what]}"
  assert int(ran["same"]["nefc_max"]) == sc.DIM[SENSOR_SCENE] and float(ran["same"]["force_max"]) > 0


def test_contact_sensor_wrench_slots(ran):
  out = ran["sensor"]
  adr, dim = out["sensor_adr"].tolist(), out["sensor_dim"].tolist()
  assert dim == [1, 3, 3, 2, 6, 6]
  sd = out["step_sensordata"].reshape(sc.NWORLD, -1)
  force = out["step_contact_force"].reshape(sc.NWORLD, -1, 3)[:, 0]
  torque = out["step_contact_torque"].reshape(sc.NWORLD, -1, 3)[:, 0]
  ncon = out["step_ncon"].reshape(-1)
  assert all(np.any(torque[:, k] != 0) and np.any(force[:, k] != 0) for k in range(3))
  for k0 in (0, 3):  # the one-slot sensor, then slot 0 of the two-slot one (slot 1: no contact)
    assert np.array_equal(sd[:, adr[k0]], (ncon > 0).astype(np.float32))
    assert np.array_equal(sd[:, adr[k0 + 1]:adr[k0 + 1] + 3], force)
    assert np.array_equal(sd[:, adr[k0 + 2]:adr[k0 + 2] + 3], torque)
  assert not np.any(sd[:, adr[5] + 3:adr[5] + 6]) and not np.any(sd[:, adr[4] + 3:adr[4] + 6])


def test_sliding_rollout(ran):
  out = ran["rollout"]
  h, f0, g = sc.H, sc.ROLLOUT_FRICTION, 9.81
  q0, v0, d = sc.rollout_start()
  v0 = np.asarray(v0, np.float32).astype(float)
  qs_ref, vs_ref, amax = sc.rollout_reference()
  vstep = 2e-3 * np.maximum(1.0, amax) * h + 1e-5
  pstep = 2e-3 * np.maximum(1.0, amax) * h * h + 1e-5
  q, v = out["qpos"].astype(float), out["qvel"].astype(float)
  speed = np.linalg.norm(v[:, :2], axis=1)
  k = np.arange(sc.ROLLOUT_STEPS)
  sliding = speed > 0.05
  last = int(np.argmin(sliding))
  assert last >= 20 and not sliding[-50:].any(), f"the puck slides for {last} steps"
  fall = np.linalg.norm(v0[:2]) - speed
  want = f0 * (g * (k + 1) * h + v[:, 2] - v0[2])
  c = _ratio((fall - want)[:last], (1.0 + f0) * np.cumsum(vstep)[:last])
  print(f"rollout: slid {last} steps, momentum identity {c:.3f} of the accumulated bound")
  assert c <= 1.0
  # lateral drift: across the initial direction, in the plane
  across = np.array([-d[1], d[0]])
  drift = np.abs((q[:, :2] - np.asarray(q0, np.float32)[:2].astype(float)) @ across)
  drift_ref = np.abs((qs_ref[:, :2] - np.asarray(q0, np.float32)[:2].astype(float)) @ across)
  bound = drift_ref.max() + sc.ROLLOUT_STEPS * pstep.max()
  print(f"rollout: lateral drift {drift.max():.3e} (reference {drift_ref.max():.3e}) of {bound:.3e}")
  assert drift.max() <= bound
  assert speed[-1] <= np.cumsum(vstep)[-1]
