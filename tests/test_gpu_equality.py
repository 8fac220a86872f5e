"""The engine's joint equality rows on the scenes of tests/equality_scenes.py against the fp64
reference tests/equality_ref.py (which shares no code with the engine; the oracle ignores
equalities and only supplies qM, qacc_smooth and the integration where a scene's M is coupled).

Six scenes at batch sizes 1 and 70 on the generic kernels (`specialize="never"`; a model with
equalities has no other kernels), one forward() and one step() each, one GPU child process for
the whole module (tests/equality_child.py).  Per world, against the reference:

  nefc                 2 (active equalities) + limit rows + contact rows; ncon equal
  qacc                 B_a = 2e-3 max(1, max|qacc|)                              test_gpu_parity
                       a world outside it: 1e-4 + 1024 eps32 s_i per dof         test_gpu_model_zoo
                       (s_i: equality_scenes.qacc_scale, oracle_lib.qacc_error_scale's rule
                       with the equality rows always active)
  qvel / qpos          h x / h^2 x the qacc bound + 1e-5                         test_gpu_parity
  qfrc_constraint_j    sum_i |J_ij| e_i, e_i = D_i sum_j |J_ij| B_a + 32 eps32 D_i (|aref_i| +
                       sum_j |J_ij| |a_j|)                        test_gpu_constraint_params
                       (mixed_many: the pair's two dofs; the legged dofs' rows are the oracle's)
  contact_force        mixed: against constraint_ref, that module's force bound (normal
                       sum_i e_i, tangent k mu (e_2k + e_2k+1) over the contact's rows)

Further: quartic with eq_data / eq_solref / eq_solimp expanded but left at the model's values
equals the unexpanded sim bit for bit in parity_util.DATA_FIELDS; on gripper step(4), four
step(1) and a replayed graph of step(4) are bit-identical; and a 200-step rollout of gripper
under a sinusoidal position target of the left finger keeps the engine's largest |q_l + q_r|
within the reference rollout's largest plus 200 x the per-step qpos bound above.

Largest err / bound per scene, measured on an MI355X against the reference (batch 70; batch 1 is
world 0 of the same states, and no larger anywhere):
  scene        rows    Newton iterations   qacc   qvel   qpos   qfrc   cforce
  slide_pair   2       <= 2                0.005  0.003  0.001  0.000  -
  quartic      2       <= 2                0.003  0.002  0.007  0.001  -
  lock         2       1                   0.002  0.002  0.002  0.000  -
  gripper      2..4    <= 3                0.000  0.002  0.004  0.000  -
  mixed        3..8    <= 2                0.006  0.018  0.013  0.000  0.000
  mixed_many   6..98   <= 9                0.003  0.002  0.007  0.000  -
(no world needed the fp32 model; the force ratios are small because the first term of the bound,
D |J| x the qacc bound, is far above the measured error, as test_gpu_constraint_params notes.)
Gripper rollout, 200 steps: the engine's largest |q_l + q_r| 9.733e-04, the reference rollout's
9.733e-04, 200 x the per-step qpos bound 2.079e-03.

A child that is killed at its time limit, exits with 134 / 139 / a negative status or reports a
HIP illegal access sets a module flag; every later test fails without starting anything.
Child time limit: the child took 2.5 s on an MI355X, most of it interpreter start-up; ten times
that is 25 s, so the 30 s the module started with stand: CHILD_TIMEOUT = 30 s.
"""

from __future__ import annotations

import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import equality_scenes as es

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 30  # seconds (module docstring)
BATCHES = (1, es.NWORLD)
EPS32 = float(np.finfo(np.float32).eps)
QACC_FLOOR, QACC_EPS_MUL = 1e-4, 1024.0  # tests/test_gpu_rollout_parity.py
FORCE_C = 32.0  # x eps32: tests/test_gpu_constraint_params.py

_faulted = []  # the module flag: why no further child may start


def _run_child(tmp):
  if _faulted:
    pytest.fail(f"not run: an earlier child faulted ({_faulted[0]})")
  job = os.path.join(tmp, "job.json")
  out = os.path.join(tmp, "out")
  os.makedirs(out, exist_ok=True)
  with open(job, "w") as fh:
    json.dump({"scenes": list(es.SCENES), "batches": list(BATCHES), "same": "quartic", "paths": "gripper",
               "rollout": "gripper"}, fh)
  cmd = [sys.executable, os.path.join(HERE, "equality_child.py"), job, out]
  t0 = time.perf_counter()
  try:
    r = subprocess.run(cmd, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
  except subprocess.TimeoutExpired as e:
    done = (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
    _faulted.append(f"killed at its {CHILD_TIMEOUT} s limit after: {done[-200:]}")
    pytest.fail(f"child hung: {_faulted[0]}")
  print(f"equality child took {time.perf_counter() - t0:.1f} s")
  text = (r.stdout or "") + (r.stderr or "")
  if r.returncode in (134, 139) or r.returncode < 0 or "illegal memory access" in text:
    _faulted.append(f"exit status {r.returncode} after: {(r.stdout or '')[-200:]}")
    pytest.fail(f"child faulted ({r.returncode}):\n{text[-3000:]}")
  assert r.returncode == 0, f"child failed ({r.returncode}):\n{text[-3000:]}"
  res = {}
  for name in [f"{s}_{n}" for s in es.SCENES for n in BATCHES] + ["same", "paths", "rollout"]:
    with np.load(os.path.join(out, f"{name}.npz")) as z:
      res[name] = {k: z[k] for k in z.files}
  return res


@pytest.fixture(scope="module")
def ran(gpu_device, tmp_path_factory):
  return _run_child(str(tmp_path_factory.mktemp("equality")))


def _ratio(err, bound):
  err, bound = np.abs(np.asarray(err, float)), np.asarray(bound, float)
  if not err.size:
    return 0.0
  return float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-300))))


def check_scene(name, n, out):
  """Every per-world comparison of the module docstring; returns the largest ratios."""
  h = es.H
  m = es.model(name)
  R = dict(qacc=0.0, qacc_fp32=0.0, qvel=0.0, qpos=0.0, qfrc=0.0, cforce=0.0)
  bad, nfallback = [], 0

  def expect(ok, msg):
    if not ok:
      bad.append(msg)

  neq_active = int(np.sum(m.arrays["eq_active0"]))
  for w in range(n):
    t = {k[5:]: v[w] for k, v in out.items() if k.startswith("step_")}
    ncon, nefc = int(t["ncon"].reshape(-1)[0]), int(t["nefc"].reshape(-1)[0])
    frame = t["contact_frame"].reshape(-1, 9)[0].astype(float) if name == "mixed" and ncon else None
    r = es.reference(name, w, frame=frame)
    assert r["nefc"] == 2 * neq_active + r.get("nlim", 0) + r.get("ncrow", 0) or name == "mixed_many"
    fw = (int(out["fwd_ncon"][w].reshape(-1)[0]), int(out["fwd_nefc"][w].reshape(-1)[0]))
    expect(fw == (r["ncon"], r["nefc"]), f"world {w}: forward ncon / nefc {fw} vs {r['ncon']} / {r['nefc']}")
    same = (ncon, nefc) == (r["ncon"], r["nefc"])
    expect(same, f"world {w}: step ncon / nefc {ncon} / {nefc} vs {r['ncon']} / {r['nefc']}")
    if not same:
      continue
    sc = max(1.0, float(np.abs(r["qacc"]).max()))
    ea = np.abs(t["qacc"] - r["qacc"])
    ra = _ratio(ea, 2e-3 * sc)
    R["qacc"] = max(R["qacc"], ra)
    if ra <= 1.0:
      ab = np.full(ea.size, 2e-3 * sc)
    else:  # outside the test_gpu_parity bound: the per-dof fp32 model must explain it
      nfallback += 1
      ab = QACC_FLOOR + QACC_EPS_MUL * EPS32 * es.qacc_scale(name, w)
      rf = _ratio(ea, ab)
      R["qacc_fp32"] = max(R["qacc_fp32"], rf)
      expect(rf <= 1.0, f"world {w}: qacc {ra:.2f} of the parity bound and {rf:.2f} of the fp32 model")
    c = _ratio(t["qvel"] - r["qvel"], ab * h + 1e-5)
    expect(c <= 1.0, f"world {w}: qvel {c:.2f} of its bound")
    R["qvel"] = max(R["qvel"], c)
    c = _ratio(t["qpos"] - r["qpos"], ab.max() * h * h + 1e-5)
    expect(c <= 1.0, f"world {w}: qpos {c:.2f} of its bound")
    R["qpos"] = max(R["qpos"], c)
    # ---- forces: per row e_i = D_i |J_i| ab + c eps32 D_i (|aref_i| + |J_i| |a|)
    J, D = r["Jmag"], r["D"]
    e = D * (J @ ab) + FORCE_C * EPS32 * D * (np.abs(r["aref"]) + J @ np.abs(r["qacc"]))
    dofs = slice(es.NLEG_DOF, None) if name == "mixed_many" else slice(None)
    c = _ratio((t["qfrc_constraint"] - r["qfrc_constraint"])[dofs], (J.T @ e)[dofs])
    expect(c <= 1.0, f"world {w}: qfrc_constraint {c:.2f} of its bound")
    R["qfrc"] = max(R["qfrc"], c)
    if name == "mixed":
      gf = t["contact_force"].reshape(-1, 3)[0].astype(float)
      ec = e[len(e) - r["ncrow"]:] if r["ncrow"] else np.zeros(0)
      mu = r["mu"]
      bound = np.array([ec.sum(), mu * (ec[0] + ec[1]), mu * (ec[2] + ec[3])]) if ec.size == 4 else np.zeros(3)
      expect(np.all(gf[bound == 0] == 0.0), f"world {w}: contact_force {gf} without an active row")
      c = _ratio(gf - r["contact_force"], bound)
      expect(c <= 1.0, f"world {w}: contact_force {c:.2f} of its bound")
      R["cforce"] = max(R["cforce"], c)
  nefcs = out["step_nefc"].reshape(-1)
  print(f"{name} x {n}: nefc {int(nefcs.min())}..{int(nefcs.max())} niter max {int(out['step_solver_niter'].max())} "
        f"fallback worlds {nfallback} ratios " + " ".join(f"{k} {v:.3f}" for k, v in R.items()))
  assert not bad, f"{name} x {n}: {len(bad)} mismatches, first: " + "; ".join(bad[:6])
  return R


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("name", es.SCENES)
def test_engine_matches_the_reference(name, n, ran):
  out = ran[f"{name}_{n}"]
  assert out["info"][0] == 0 and out["info"][1] == 0, "an equality model ran a specialised kernel"
  assert out["step_nefc"].shape[0] == n
  check_scene(name, n, out)


def test_expanded_fields_at_model_values_change_nothing(ran):
  rep = json.loads(str(ran["same"]["same"]))
  for what in ("fwd", "step"):
    assert not rep[what]["fields"], f"quartic: expanded eq fields at the model's values differ after {what}: {rep[what]}"
  assert int(ran["same"]["nefc_min"]) == 2


def test_step_paths_are_bit_identical(ran):
  rep = json.loads(str(ran["paths"]["paths"]))
  for what in ("single", "graph"):
    assert not rep[what]["fields"], f"gripper: step(4) differs from {what}: {rep[what]}"
  assert int(ran["paths"]["nefc_max"]) >= 3 and float(ran["paths"]["moved"]) > 0.0


def test_gripper_rollout_holds_the_coupling(ran):
  ref_worst, amax = es.rollout_reference()
  got = float(ran["rollout"]["worst"].max())
  step_bound = es.H * es.H * 2e-3 * max(1.0, amax) + 1e-5
  print(f"gripper rollout: engine max |q_l + q_r| {got:.3e}, reference {ref_worst:.3e}, "
        f"{es.ROLLOUT_STEPS} x per-step qpos bound {es.ROLLOUT_STEPS * step_bound:.3e}")
  assert np.isfinite(got)
  assert got <= ref_worst + es.ROLLOUT_STEPS * step_bound
