"""The engine's torsional and rolling friction rows (contacts of dimension 4 and 6) on the probe
scenes of tests/condim_scenes.py against the independent fp64 reference tests/condim_ref.py.
The oracle does not know condim > 3: these scenes are held to the reference only.

Five scenes x 32 worlds on the generic kernels (`specialize="never"`), one forward() and one
step() per scene, one GPU child process for the whole module (tests/condim_child.py).  Every
world has its own copy of geom_friction (three distinct components), geom_solref, geom_solimp
and geom_margin, written after expand_model_fields.

Per world of the four reference scenes, with the reference taking one engine output, the
contact frame's tangents, after checking the frame (constraint_ref.check_frame), and the bounds
of tests/test_gpu_constraint_params.py extended to the added rows (condim_scenes.force_bounds):

  ncon nefc            equal (tie clearance 2e-4)
  contact_dist         atol 2e-5
  qacc                 B_a = 2e-3 max(1, max|qacc|)
  qvel / qpos          h x / h^2 x the qacc bound + 1e-5
  efc row force f_i    e_i = D_i sum_j |J_ij| B_a + c eps32 D_i (|aref_i| + sum_j |J_ij| |a_j|)
  qfrc_constraint_j    sum_i |J_ij| e_i   (row-derived: the reference's J' f)
  contact_force        normal sum_i e_i (all 2 (dim - 1) rows), tangent k mu_k (e_2k + e_2k+1)
  contact_torque       component k - 2: mu_k (e_2k + e_2k+1), k = 2, 3, 4
  stats()["unsupported"] == 0

c starts from that module's FORCE_C = 32 eps32.  Measured multiples of eps32 on an MI355X
(MEASURED below): spin_plane4 2.6, spin_plane6 1.3 (the same at 1 and 70 worlds), two_balls6 1.1,
hinge_pad6 10.1.  None exceeds 16, so c = 32 stands (above 16 it would become the next power of
two above twice the measurement, which is how that module derived 32).

Largest err / bound per scene, measured on an MI355X:
  scene         rows    dist   qacc   qvel   qpos   qfrc   cforce ctorque  wrench
  spin_plane4   0, 6    0.003  0.010  0.017  0.012  0.000  0.000  0.000    0.000
  spin_plane6   0, 10   0.002  0.008  0.026  0.011  0.000  0.000  0.000    0.000
  two_balls6    0, 10   0.002  0.002  0.004  0.013  0.000  0.000  0.000    0.000
  hinge_pad6    0, 10   0.001  0.003  0.005  0.002  0.000  0.001  0.003    0.000
  many70        106     -      -      -      -      -      -      -        0.007
(the force ratios are small for the reason given in tests/test_gpu_constraint_params.py: the
first term of the bound, D |J| x the qacc bound, is far above the measured error.)

Wrench consistency, on every scene and the only physics check on many70: in fp64 from the
engine's own outputs, for a free body qfrc_constraint[:3] = sum F_world and qfrc_constraint[3:6]
= R' sum (r x F + T), body 1 of a contact taking the opposite wrench (two_balls6), and through
the hinge qfrc = u . (r x F + T) (hinge_pad6).  It compares phase B's J' f with phase C's decode,
so a sign or scale error in either shows.  The bound is the sum of the per-contact force bounds:
on the reference scenes the three contact_force bounds summed (moments: x |r|, plus the three
contact_torque bounds); on many70, which has no reference, both sides are fp32 sums of the same
row forces, every term of which is a product of at most a dozen rounded factors, so the bound is
FORCE_C eps32 x the summed magnitudes sum_c f_n (1 + 2 mu_0) (moments: x |r|, plus f_n (mu_2 + 2
mu_3)) with a floor of 1e-6 of the largest.  many70 also asserts 70 contacts and 106 rows in every
world, re-solved at max capacity (stats()["resolved"]) with nothing dropped (no overflow event).

Batch shapes: spin_plane6 again at 1 world and at 70 worlds against the reference, and step(4)
against four step(1) and a captured, replayed step(4), bit for bit.  Contact sensor: the
`torque` slot of a one-slot (wave form) and a two-slot (serial form) sensor equals contact_torque
of the selected contact, as the `force` slot equals contact_force (contact frame, no sign).
Expanded fields at model values: bit-identical over parity_util.DATA_FIELDS plus contact_torque.

Spin-down rollout: 200 steps of an isotropic ball spinning at 10 rad/s about the normal of a
level plane.  With condim 3 the spin changes by less than the summed per-step qvel bounds; with
condim 4 it follows the reference's own rollout within the bound summed up to each step, for as
long as the active set the reference finds at the engine's state equals the one of its own
rollout, and ends below 5 % of the initial spin (the reference alone is there well before step
150: tests/test_condim.py).

A child that is killed at its time limit, exits with 134 / 139 / a negative status or reports a
HIP illegal access sets a module flag; every later test fails without starting anything.
Child time limit: the child took 3.1 s on an MI355X, most of it interpreter start-up; ten times
that: CHILD_TIMEOUT = 31 s.
"""

from __future__ import annotations

import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import condim_scenes as sc
import constraint_ref as cr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# the child took 3.1 s on an MI355X (most of it interpreter start-up and the sims' creation);
# ten times that
CHILD_TIMEOUT = 31
EPS32 = sc.EPS32
FORCE_C = sc.FORCE_C
BATCHES = {"spin_plane6": [sc.NWORLD, 1, 70]}
# largest error / (eps32 x the magnitude of the terms summed) per scene, MI355X
MEASURED = {"spin_plane4": 2.6, "spin_plane6": 1.3, "two_balls6": 1.1, "hinge_pad6": 10.1}

_faulted = []  # the module flag: why no further child may start


def _run_child(tmp):
  if _faulted:
    pytest.fail(f"not run: an earlier child faulted ({_faulted[0]})")
  job = os.path.join(tmp, "job.json")
  out = os.path.join(tmp, "out")
  os.makedirs(out, exist_ok=True)
  with open(job, "w") as fh:
    json.dump({"scenes": list(sc.SCENES), "batches": BATCHES, "paths": ["spin_plane6", [1, 70]],
               "sensor": "spin_plane6", "same": "spin_plane6", "rollout": True}, fh)
  cmd = [sys.executable, os.path.join(HERE, "condim_child.py"), job, out]
  t0 = time.perf_counter()
  try:
    r = subprocess.run(cmd, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
  except subprocess.TimeoutExpired as e:
    done = (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
    _faulted.append(f"killed at its {CHILD_TIMEOUT} s limit after: {done[-200:]}")
    pytest.fail(f"child hung: {_faulted[0]}")
  print(f"condim child took {time.perf_counter() - t0:.1f} s")
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
  return _run_child(str(tmp_path_factory.mktemp("condim")))


def _ratio(err, bound):
  err, bound = np.abs(np.asarray(err, float)), np.asarray(bound, float)
  if not err.size:
    return 0.0
  return float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-300))))


def _world(out, w):
  return {k[5:]: v[w] for k, v in out.items() if k.startswith("step_")}


def check_scene(name, out, n):
  """Every comparison of the module docstring for one scene against the reference; returns the
  largest ratios and the measured multiple of eps32."""
  h = sc.H
  R = dict(dist=0.0, qacc=0.0, qvel=0.0, qpos=0.0, qfrc=0.0, cforce=0.0, ctorque=0.0)
  cmeas, bad, nrows = 0.0, [], set()

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
    if ncon:
      for dk in (t["contact_dist"].reshape(-1)[0], out["fwd_contact_dist"][wi].reshape(-1)[0]):
        c = _ratio(dk - r["dist"], 2e-5)
        expect(c <= 1.0, f"world {wi}: contact_dist {c:.2f} x 2e-5")
        R["dist"] = max(R["dist"], c)
    ab = np.full(r["qacc"].size, 2e-3 * max(1.0, float(np.abs(r["qacc"]).max())))
    for key, got, bound in (("qacc", t["qacc"], ab), ("qvel", t["qvel"], ab * h + 1e-5),
                            ("qpos", t["qpos"], ab.max() * h * h + 1e-5)):
      c = _ratio(got - r[key], bound)
      expect(c <= 1.0, f"world {wi}: {key} {c:.2f} of its bound")
      R[key] = max(R[key], c)
    b = sc.force_bounds(r, ab)
    errs = [(t["qfrc_constraint"] - r["qfrc_constraint"], b["qfrc"], "qfrc"),
            (t["contact_force"].reshape(-1, 3)[0].astype(float) - r["contact_force"], b["force"], "cforce"),
            (t["contact_torque"].reshape(-1, 3)[0].astype(float) - r["contact_torque"], b["torque"], "ctorque")]
    for err, (b_first, b_mag), key in errs:
      cmeas = max(cmeas, _ratio(err, EPS32 * b_mag) if np.any(b_mag > 0) else 0.0)
      expect(np.all(np.abs(err)[b_mag == 0] == 0.0), f"world {wi}: {key} {err} without an active row")
      c = _ratio(err, b_first + FORCE_C * EPS32 * b_mag)
      expect(c <= 1.0, f"world {wi}: {key} {c:.2f} of its bound")
      R[key] = max(R[key], c)
    # the other contact slots stay empty
    expect(not np.any(t["contact_torque"].reshape(-1, 3)[1:]), f"world {wi}: torque past the contact")
  print(f"{name} x {n}: nefc {sorted(nrows)} measured c {cmeas:.1f} ratios " + " ".join(f"{k} {v:.3f}" for k, v in R.items()))
  assert not bad, f"{name} x {n}: {len(bad)} mismatches, first: " + "; ".join(bad[:6])
  assert nrows == {0, 2 * (sc.MAX_CONDIM[name] - 1)} or n == 1
  return R, cmeas


@pytest.mark.parametrize("name,n", [(s, sc.NWORLD) for s in sc.REF_SCENES] + [("spin_plane6", 1), ("spin_plane6", 70)])
def test_engine_matches_the_reference(name, n, ran):
  out = ran[f"{name}_{n}"]
  assert out["info"][0] == 0 and out["info"][1] == 0, "specialize='never' ran a specialised kernel"
  assert out["stats"][4] == 0, "stats()['unsupported']: a contact was counted as an unsupported pair"
  assert not np.any(out["reset_wrench_max"]), "reset left a contact force or torque"
  check_scene(name, out, n)


# ----------------------------------------------------------------------------- wrench consistency
def _wrench_check(name, out):
  m = sc.model(name)
  q0 = sc.states(name)[0].astype(np.float32).astype(float)
  fr = sc.fields(name)["geom_friction"]
  prio = np.asarray(m.arrays["geom_priority"])
  gbody = np.asarray(m.arrays["geom_bodyid"])
  worst = 0.0
  for w in range(sc.NWORLD):
    t = _world(out, w)
    ncon = int(t["ncon"].reshape(-1)[0])
    nv = t["qfrc_constraint"].size
    want, bound = np.zeros(nv), np.zeros(nv)
    for c in range(ncon):
      F = t["contact_frame"].reshape(-1, 3, 3)[c].astype(float)
      f, tq = t["contact_force"].reshape(-1, 3)[c].astype(float), t["contact_torque"].reshape(-1, 3)[c].astype(float)
      pos = t["contact_pos"].reshape(-1, 3)[c].astype(float)
      g1, g2 = (int(x) for x in t["contact_geom"].reshape(-1, 2)[c])
      Fw, Tw = F.T @ f, F.T @ tq
      if name in sc.REF_SCENES:
        r = sc.reference(name, w, frame=F.reshape(-1))
        ab = np.full(r["qacc"].size, 2e-3 * max(1.0, float(np.abs(r["qacc"]).max())))
        b = sc.force_bounds(r, ab)
        bf = float(np.sum(b["force"][0] + FORCE_C * EPS32 * b["force"][1]))
        bt = float(np.sum(b["torque"][0] + FORCE_C * EPS32 * b["torque"][1]))
      else:  # both sides sum the same fp32 row forces: the rounding of the summed magnitudes
        f3 = fr[w, g1] if prio[g1] > prio[g2] else fr[w, g2] if prio[g2] > prio[g1] else np.maximum(fr[w, g1], fr[w, g2])
        bf = FORCE_C * EPS32 * f[0] * (1.0 + 2.0 * f3[0])
        bt = FORCE_C * EPS32 * f[0] * (f3[1] + 2.0 * f3[2])
      for g, sgn in ((g2, 1.0), (g1, -1.0)):
        b = int(gbody[g])
        if b == 0:
          continue
        if name == "hinge_pad6":
          u, rr = sc._unit(sc.PAD["axis"]), pos - sc._pad_anchor()
          want[0] += sgn * float(u @ (np.cross(rr, Fw) + Tw))
          bound[0] += np.linalg.norm(rr) * bf + bt
        else:
          a = 7 * (b - 1 if name == "two_balls6" else 0)
          d = 6 * (b - 1 if name == "two_balls6" else 0)
          rr = pos - q0[w, a:a + 3]
          Rb = cr.quat_mat(q0[w, a + 3:a + 7])
          want[d:d + 3] += sgn * Fw
          want[d + 3:d + 6] += sgn * (Rb.T @ (np.cross(rr, Fw) + Tw))
          bound[d:d + 3] += bf
          bound[d + 3:d + 6] += np.linalg.norm(rr) * bf + bt
    if name == "many70":
      bound = np.maximum(bound, 1e-6 * bound.max())
    got = t["qfrc_constraint"].astype(float)
    assert np.all(got[bound == 0] == want[bound == 0]), f"{name} world {w}: qfrc {got} without a force"
    c = _ratio(got - want, bound)
    worst = max(worst, c)
    assert c <= 1.0, f"{name} world {w}: qfrc_constraint {got} vs the contacts' wrench {want}: {c:.2f} of the bound"
  print(f"{name}: wrench consistency, largest err / bound {worst:.3f}")


@pytest.mark.parametrize("name", sc.SCENES)
def test_wrench_consistency(name, ran):
  out = ran[f"{name}_{sc.NWORLD}"]
  if name == "many70":
    assert np.all(out["step_ncon"].reshape(-1) == 70) and np.all(out["step_nefc"].reshape(-1) == 106)
    assert np.all(out["fwd_ncon"].reshape(-1) == 70) and np.all(out["fwd_nefc"].reshape(-1) == 106)
    st = dict(zip(("max_ncon", "max_nefc", "con_overflow", "row_overflow", "unsupported", "resolved"), out["stats"]))
    assert st["resolved"] >= sc.NWORLD, f"the worlds were not re-solved at max capacity: {st}"
    assert st["con_overflow"] == 0 and st["row_overflow"] == 0 and st["unsupported"] == 0, st
    assert (st["max_ncon"], st["max_nefc"]) == (70, 106), st
    cd = np.asarray(sc.model(name).arrays["geom_condim"])
    tq = out["step_contact_torque"].reshape(sc.NWORLD, -1, 3)
    g2 = out["step_contact_geom"].reshape(sc.NWORLD, -1, 2)[:, :70, 1]
    assert not np.any(tq[:, :70][cd[g2] == 1]) and np.any(tq[:, :70][cd[g2] == 6])
  _wrench_check(name, out)


# ----------------------------------------------------------------------------- paths, sensor
@pytest.mark.parametrize("n", [1, 70])
def test_step_paths_are_bit_identical(n, ran):
  out = ran[f"paths_{n}"]
  rep = json.loads(str(out["paths"]))
  for k in ("single", "graph"):
    assert not rep[k]["fields"], f"{n} worlds: step(4) differs from {k}: {rep[k]}"
  assert int(out["nefc_max"]) == 10 and float(out["moved"]) > 1e-4


def test_contact_sensor_torque_slot(ran):
  out = ran["sensor"]
  adr, dim = out["sensor_adr"].tolist(), out["sensor_dim"].tolist()
  assert dim == [1, 3, 3, 2, 6, 6]
  sd = out["step_sensordata"].reshape(sc.NWORLD, -1)
  force = out["step_contact_force"].reshape(sc.NWORLD, -1, 3)[:, 0]
  torque = out["step_contact_torque"].reshape(sc.NWORLD, -1, 3)[:, 0]
  ncon = out["step_ncon"].reshape(-1)
  assert np.any(torque[:, 0] != 0) and np.any(torque[:, 1] != 0) and np.any(torque[:, 2] != 0)
  for k0 in (0, 3):  # the one-slot sensor, then slot 0 of the two-slot one (slot 1: no contact)
    assert np.array_equal(sd[:, adr[k0]], (ncon > 0).astype(np.float32))
    assert np.array_equal(sd[:, adr[k0 + 1]:adr[k0 + 1] + 3], force)
    assert np.array_equal(sd[:, adr[k0 + 2]:adr[k0 + 2] + 3], torque)
  assert not np.any(sd[:, adr[5] + 3:adr[5] + 6]) and not np.any(sd[:, adr[4] + 3:adr[4] + 6])


def test_expanded_fields_at_model_values_change_nothing(ran):
  rep = json.loads(str(ran["same"]["same"]))
  for what in ("fwd", "step"):
    assert not rep[what]["fields"], f"expanded fields at the model's values differ after {what}: {rep[what]}"
  assert int(ran["same"]["nefc_max"]) == 10 and float(ran["same"]["torque_max"]) > 0


# ----------------------------------------------------------------------------- spin-down rollout
def _spin(q, v):
  return np.array([float((cr.quat_mat(q[k, 3:7].astype(float)) @ v[k, 3:6].astype(float))[2]) for k in range(len(q))])


def test_spin_down_rollout(ran):
  out = ran["rollout"]
  assert out["spin_down3_unsupported"] == 0 and out["spin_down4_unsupported"] == 0
  h = sc.H
  q0, v0 = (np.asarray(x, np.float32) for x in sc.spin_down_start())
  for name in ("spin_down3", "spin_down4"):
    om_ref, sets, amax = sc.spin_down_reference(name)
    step_bound = 2e-3 * np.maximum(1.0, amax) * h + 1e-5
    acc = np.cumsum(step_bound)
    q, v = out[name + "_qpos"], out[name + "_qvel"]
    om = _spin(q, v)
    if name == "spin_down3":
      c = _ratio(om - sc.SPIN_OMEGA, acc)
      print(f"spin_down3: largest spin change / accumulated bound {c:.3f}")
      assert c <= 1.0, f"the condim-3 ball's spin changed: {om[[0, 50, 199]]}"
      continue
    worst, agreed = 0.0, 0
    for k in range(sc.ROLLOUT_STEPS):
      qk, vk = (q0, v0) if k == 0 else (q[k - 1], v[k - 1])
      r = sc.reference(name, 0, q=qk.astype(float), qv=vk.astype(float))
      if tuple((r["efc_force"] > 0).tolist()) != sets[k]:
        break
      agreed += 1
      c = _ratio(om[k] - om_ref[k], acc[k])
      worst = max(worst, c)
      assert c <= 1.0, f"step {k}: spin {om[k]} vs the reference's {om_ref[k]}: {c:.2f} of the accumulated bound"
    print(f"spin_down4: active sets agreed for {agreed} steps, largest err / bound {worst:.3f}, final spin {om[-1]:.3e}")
    assert agreed >= 5
    assert abs(om_ref[149]) < 0.05 * sc.SPIN_OMEGA  # the reference alone is there by step 150
    assert abs(om[-1]) < 0.05 * sc.SPIN_OMEGA, f"the condim-4 ball still spins at {om[-1]}"
