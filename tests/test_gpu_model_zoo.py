"""The step kernels on the synthetic model zoo (tests/model_zoo.py) against the fp64 oracle.

Every zoo model the engine admits (zoo.RUNNABLE) runs on the generic kernels
(`specialize="never"`): all ten register-row lengths of csrc/engine.hip, padding lanes at every
dof count mod 4, 60 dofs on 60 bodies, a 24-level chain, bodies with two and three joints and
with five, six, seven and sixteen children, slides and joint springs, constraint rows on
both sides of 64, and (`params14`, `params38`) non-default contact and limit parameters with
contacts in their gap and both rows of a limit at once.  16 worlds per model (32 for rows64),
one GPU child process for the whole module (tests/zoo_child.py); `fallbacks26` runs once more on its run-time specialised kernels,
which __graft_entry__.build() compiled into the in-tree cache (no compile happens here).  The
models of zoo.REJECTED (more than 60 dofs, a tree after a tree of several bodies) are refused
by mjx_model_create and launch nothing: tests/test_model_zoo_cpu.py asserts the refusals.

Compared after `forward()` with the oracle's forward, after `step()` with its step:

  field                         bound                                        from
  xpos xipos subtree_com xquat  atol 2e-5 (xquat up to sign)                 test_gpu_parity
  cvel                          atol 1e-4 + 1e-4 |v|                         test_gpu_parity
  qacc_smooth                   1e-3 max(1, max|qacc_smooth|) per world      test_gpu_parity
  qfrc_bias qfrc_passive        atol 1e-3 + 1e-4 |f|                         test_gpu_parity's
  actuator_force                atol 1e-3 + 1e-4 |f|                           force bound
  sensordata                    3e-3 max(1, max|s|) per world                test_gpu_parity
  ncon nefc                     equal (no sampled contact within 1e-4 of its activation
                                distance: tests/test_model_zoo_cpu.py)
  M (Simulation.mass_matrix)    4 eps32 x the magnitude of the CRB terms summed, per entry
                                (oracle_lib.mass_matrix_scale)               test_gpu_rollout_parity
                                + 4 eps32 sqrt(M_ii M_jj) where i or j is a linear dof   see below
  qacc                          2e-3 max(1, max|qacc|) per world             test_gpu_parity
  qvel / qpos                   h x / h^2 x the qacc bound + 1e-5            test_gpu_parity
  solver_niter                  within 1                                     test_gpu_parity

The mass matrix: tests/test_gpu_rollout_parity.py bounds an entry by 4 eps32 x the magnitude of
the terms the CRB sum adds up.  That covers the rounding of the sum, not of its inputs, and on
the robots the two are alike.  That bound is asserted as it stands on every entry between two
rotational dofs (hinges, a free joint's rotations; measured at most 0.13 of it).  A linear dof (a
slide, a free joint's translation) has a pure direction for its spatial axis: a slide's M entry
against a free joint's translation is a single term, (subtree mass) x (one world component of
the slide axis), and against another slide (subtree mass) x (the two axes' dot product); where
the axes are near orthogonal the term's magnitude vanishes while the axis, a unit vector turned to the world by a
chain of fp32 quaternion products, still carries eps32-sized absolute error per component (the
zoo measured 544 x the term bound on such an entry, 1.6e-7 absolute on a matrix whose diagonal
there is 13 and 1.8).  M_ij = c_i' I_c c_j with the dofs' spatial axes c, so a relative error d
of each axis moves it by at most 2 d sqrt(M_ii M_jj) (Cauchy-Schwarz in the I_c inner product);
with d = 2 eps32 (a rotation by a rounded quaternion) the bound of an entry with a linear dof
gains 4 eps32 sqrt(M_ii M_jj).  Neither term comes from the engine's output.

A world whose qacc misses the test_gpu_parity bound is held to the per-dof fp32 model of
test_gpu_rollout_parity instead: 1e-4 + 1024 eps32 s_i, s_i = oracle_lib.qacc_error_scale (the
oracle's |H^-1| times the magnitudes of the gradient's terms; nothing of the engine's output
enters it), and its qvel to h times that.  The ratios err / bound are printed per model.

Measured on an MI355X on this tree (largest err / bound over the model's worlds; kin = the largest
of xpos / xipos / subtree_com / xquat; M rot / M lin = entries between rotational dofs / with a
linear dof):
  model                    nv  rows    kin    cvel   smooth forces sens   M rot  M lin  qacc   qvel
  free7                     7  0..8    0.005  0.001  0.002  0.001  0.000  0.011  0.265  0.008  0.004
  free12                   12  0..8    0.006  0.001  0.004  0.002  0.005  0.020  0.266  0.002  0.001
  slide13                  13  0..2    0.013  0.002  0.002  0.002  0.001  0.027  0.403  0.001  0.001
  free16                   16  0..13   0.007  0.002  0.001  0.002  0.001  0.018  0.243  0.001  0.000
  free18                   18  1..9    0.006  0.002  0.002  0.003  0.001  0.013  0.371  0.002  0.002
  chain24                  24  0..4    0.025  0.005  0.022  0.008  0.005  0.017  0.696  0.011  0.007
  free29                   29  1..9    0.006  0.002  0.002  0.002  0.001  0.021  0.225  0.001  0.000
  free35                   35  0..15   0.007  0.002  0.004  0.002  0.001  0.023  0.494  0.002  0.002
  rows64                   38  4..96   0.007  0.002  0.001  0.003  0.003  0.039  0.063  0.008  0.005
  fixed39                  39  0..3    0.018  0.005  0.005  0.002  0.001  0.028  0.684  0.002  0.001
  free40                   40  3..22   0.008  0.003  0.003  0.002  0.002  0.024  0.579  0.002  0.000
  free45                   45  1..14   0.008  0.003  0.005  0.003  0.001  0.012  0.406  0.002  0.002
  star48                   48  1..6    0.026  0.007  0.019  0.002  0.003  0.060  0.353  0.009  0.009
  free53                   53  4..17   0.006  0.002  0.004  0.003  0.001  0.018  0.356  0.002  0.001
  fixed56                  56  1..7    0.028  0.005  0.006  0.004  0.002  0.131  0.623  0.003  0.003
  fallbacks26              26  1..24   0.007  0.002  0.005  0.002  0.002  0.022  0.406  0.003  0.003
  free57                   57  1..16   0.007  0.002  0.005  0.005  0.003  0.015  0.372  0.002  0.001
  wave60                   60  0..8    0.021  0.005  0.008  0.003  0.003  0.061  0.415  0.004  0.000
  free21                   21  0..13   0.007  0.002  0.004  0.002  0.002  0.023  0.370  0.002  0.000
  free32                   32  0..11   0.006  0.002  0.004  0.002  0.002  0.010  0.377  0.002  0.002
  free37                   37  1..13   0.007  0.002  0.006  0.004  0.004  0.020  0.295  0.005  0.005
  params14                 14  1..11   0.008  0.001  0.001  0.001  0.001  0.016  0.247  0.001  0.000
  params38                 38  3..19   0.007  0.003  0.003  0.003  0.002  0.020  0.336  0.001  0.000
  fallbacks26 (specialised) 26  1..24   0.007  0.002  0.005  0.002  0.002  0.022  0.406  0.003  0.003
(no world needed the fp32 model: the largest qacc error is 0.011 of the test_gpu_parity bound
and 0.074 of the fp32 model's.)

A four-substep step equals four single steps bit for bit (fallbacks26, wave60, and fallbacks26
on its specialised kernels).

A child that is killed at its time limit, exits with 134 / 139 / a negative status or reports
a HIP illegal access sets a module flag; every later test fails without starting anything.
Child time limit: the all-models child took 2.7 s on an MI355X (2.3 s the one-model child), most
of it interpreter start-up; the limit is ten times that: CHILD_TIMEOUT = 30 s.
"""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import model_zoo as zoo
import oracle_lib as ol
from oracle_sim import OracleData

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 30  # seconds (module docstring)
FUSED = ("fallbacks26", "wave60")
SPECIALISED = "fallbacks26"
EPS32 = float(np.finfo(np.float32).eps)
QM_EPS_MUL = 4.0  # tests/test_gpu_rollout_parity.py
QACC_FLOOR, QACC_EPS_MUL = 1e-4, 1024.0  # tests/test_gpu_rollout_parity.py
NCONMAX, NJMAX = 64, 160

_faulted = []  # the module flag: why no further child may start


def _run_child(tmp, tag, models, specialize):
  if _faulted:
    pytest.fail(f"not run: an earlier child faulted ({_faulted[0]})")
  job = os.path.join(tmp, f"{tag}.json")
  out = os.path.join(tmp, tag)
  os.makedirs(out, exist_ok=True)
  with open(job, "w") as fh:
    json.dump({"models": list(models), "specialize": specialize, "fused": list(FUSED)}, fh)
  cmd = [sys.executable, os.path.join(HERE, "zoo_child.py"), job, out]
  try:
    r = subprocess.run(cmd, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
  except subprocess.TimeoutExpired as e:
    done = (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
    _faulted.append(f"{tag}: killed at its {CHILD_TIMEOUT} s limit after: {done[-200:]}")
    pytest.fail(f"child {tag} hung: {_faulted[0]}")
  text = (r.stdout or "") + (r.stderr or "")
  if r.returncode in (134, 139) or r.returncode < 0 or "illegal memory access" in text:
    _faulted.append(f"{tag}: exit status {r.returncode} after: {(r.stdout or '')[-200:]}")
    pytest.fail(f"child {tag} faulted ({r.returncode}):\n{text[-3000:]}")
  assert r.returncode == 0, f"child {tag} failed ({r.returncode}):\n{text[-3000:]}"
  res = {}
  for name in models:
    with np.load(os.path.join(out, f"{name}.npz")) as z:
      res[name] = {k: z[k] for k in z.files}
  return res


@pytest.fixture(scope="module")
def generic(gpu_device, tmp_path_factory):
  return _run_child(str(tmp_path_factory.mktemp("zoo")), "generic", zoo.RUNNABLE, "never")


@pytest.fixture(scope="module")
def specialised(gpu_device, tmp_path_factory):
  return _run_child(str(tmp_path_factory.mktemp("zoo_spec")), "specialised", (SPECIALISED,), "auto")


_refs = {}


def oracle_refs(name):
  """fp64 references of the model's seeded worlds, computed once: forward fields (OracleData),
  one step (oracle_lib.forward), the fp32 error scales of M and of the Newton solution."""
  if name in _refs:
    return _refs[name]
  zm = zoo.get(name)
  m = zm.model
  q, qv, ctrl = zm.states()
  od = OracleData(m, NCONMAX, NJMAX)
  fwd, step, mscale, qscale = [], [], [], []
  for w in range(q.shape[0]):
    od.qpos[:], od.qvel[:], od.ctrl[:] = q[w], qv[w], ctrl[w]
    od.qacc_warmstart[:] = 0.0
    od.time = 0.0
    od.forward()
    f = {k: od.arr[k].copy() for k in ("xpos", "xquat", "xipos", "subtree_com", "cvel", "qfrc_bias",
                                       "qfrc_passive", "actuator_force", "qacc_smooth", "sensordata", "qM")}
    f["ncon"], f["nefc"] = od.ncon, od.nefc
    assert not od.overflow
    fwd.append(f)
    step.append(ol.forward(m, q[w], qv[w], None, ctrl[w], 0.0, step=True, nconmax=NCONMAX, njmax=NJMAX))
    mscale.append(ol.mass_matrix_scale(m, q[w]))
    qscale.append(ol.qacc_error_scale(m, q[w], qv[w], None, ctrl[w], 0.0, nconmax=NCONMAX, njmax=NJMAX)[0])
  _refs[name] = (fwd, step, mscale, qscale)
  return _refs[name]


def _ratio(err, bound):
  return float(np.max(np.abs(err) / bound)) if np.size(err) else 0.0


def check_model(name, out):
  """Every comparison of the module docstring for one model; returns the largest ratios."""
  zm = zoo.get(name)
  m = zm.model
  h = m.timestep
  fwd, step, mscale, qscale = oracle_refs(name)
  roots = np.asarray(m.body_rootid)
  trees = [int(r) for r in np.unique(roots[1:])]
  R = dict(kin=0.0, cvel=0.0, smooth=0.0, frc=0.0, sens=0.0, qM_rot=0.0, qM_lin=0.0, qacc=0.0, qacc_fp32=0.0,
           qvel=0.0)
  # M entries with a linear dof (a slide, a free joint's translation) in the row or the column
  lin = np.zeros(m.nv, bool)
  for j in range(m.njnt):
    d, t = int(m.jnt_dofadr[j]), int(m.jnt_type[j])
    lin[d:d + (3 if t == zoo.JNT_FREE else 1)] |= t in (zoo.JNT_FREE, zoo.JNT_SLIDE)
  linear = lin[:, None] | lin[None, :]
  tree_err = {r: 0.0 for r in trees}
  bad = []
  nfallback = 0

  def expect(ok, msg):
    if not ok:
      bad.append(msg)

  for w, (f, s) in enumerate(zip(fwd, step)):
    g = {k[4:]: v[w] for k, v in out.items() if k.startswith("fwd_")}
    expect(int(g["ncon"].reshape(-1)[0]) == f["ncon"] and int(g["nefc"].reshape(-1)[0]) == f["nefc"],
           f"world {w}: forward ncon / nefc {g['ncon']} / {g['nefc']} vs {f['ncon']} / {f['nefc']}")
    ex = np.abs(g["xpos"] - f["xpos"]).max(axis=1)
    for r in trees:
      tree_err[r] = max(tree_err[r], float(ex[roots == r].max()))
    sign = np.where((g["xquat"] * f["xquat"]).sum(axis=1, keepdims=True) < 0, -1.0, 1.0)
    kin = max(_ratio(g[k] - f[k], 2e-5) for k in ("xpos", "xipos", "subtree_com"))
    kin = max(kin, _ratio(sign * g["xquat"] - f["xquat"], 2e-5))
    expect(kin <= 1.0, f"world {w}: kinematics {kin:.2f} x 2e-5 (per-tree xpos error {tree_err})")
    R["kin"] = max(R["kin"], kin)
    c = _ratio(g["cvel"] - f["cvel"], 1e-4 + 1e-4 * np.abs(f["cvel"]))
    expect(c <= 1.0, f"world {w}: cvel {c:.2f} of its bound")
    R["cvel"] = max(R["cvel"], c)
    sc = max(1.0, float(np.abs(f["qacc_smooth"]).max()))
    c = _ratio(g["qacc_smooth"] - f["qacc_smooth"], 1e-3 * sc)
    expect(c <= 1.0, f"world {w}: qacc_smooth {c:.2f} of its bound")
    R["smooth"] = max(R["smooth"], c)
    for k in ("qfrc_bias", "qfrc_passive", "actuator_force"):
      c = _ratio(g[k] - f[k], 1e-3 + 1e-4 * np.abs(f[k]))
      expect(c <= 1.0, f"world {w}: {k} {c:.2f} of its bound")
      R["frc"] = max(R["frc"], c)
    ssc = max(1.0, float(np.abs(f["sensordata"]).max()))
    c = _ratio(g["sensordata"] - f["sensordata"], 3e-3 * ssc)
    expect(c <= 1.0, f"world {w}: forward sensordata {c:.2f} of its bound")
    R["sens"] = max(R["sens"], c)
    dg = np.sqrt(np.outer(np.diag(f["qM"]), np.diag(f["qM"])))
    eM = g["qM"] - f["qM"]
    c = _ratio(eM[~linear], QM_EPS_MUL * EPS32 * mscale[w][~linear] + 1e-12)
    expect(c <= 1.0, f"world {w}: M between rotational dofs {c:.2f} of 4 eps x its terms")
    R["qM_rot"] = max(R["qM_rot"], c)
    c = _ratio(eM[linear], QM_EPS_MUL * EPS32 * (mscale[w] + dg)[linear] + 1e-12)
    expect(c <= 1.0, f"world {w}: M with a linear dof {c:.2f} of its bound")
    R["qM_lin"] = max(R["qM_lin"], c)
    # ---- one step
    t = {k[5:]: v[w] for k, v in out.items() if k.startswith("step_")}
    same = int(t["ncon"].reshape(-1)[0]) == s["ncon"] and int(t["nefc"].reshape(-1)[0]) == s["nefc"]
    expect(same, f"world {w}: step ncon / nefc {t['ncon']} / {t['nefc']} vs {s['ncon']} / {s['nefc']}")
    if not same:
      continue
    sc = max(1.0, float(np.abs(s["qacc"]).max()))
    ea = np.abs(t["qacc"] - s["qacc"])
    fb = QACC_FLOOR + QACC_EPS_MUL * EPS32 * qscale[w]
    ra, rf = _ratio(ea, 2e-3 * sc), _ratio(ea, fb)
    R["qacc"], R["qacc_fp32"] = max(R["qacc"], ra), max(R["qacc_fp32"], rf)
    if ra <= 1.0:
      ab = np.full(m.nv, 2e-3 * sc)
    else:  # outside the test_gpu_parity bound: the per-dof fp32 model must explain it
      nfallback += 1
      ab = fb
      expect(rf <= 1.0, f"world {w}: qacc {ra:.2f} of the parity bound and {rf:.2f} of the fp32 model "
                        f"(dof {int(np.argmax(ea / fb))}, nefc {s['nefc']})")
    c = _ratio(t["qvel"] - s["qvel"], ab * h + 1e-5)
    expect(c <= 1.0, f"world {w}: qvel {c:.2f} of its bound")
    R["qvel"] = max(R["qvel"], c)
    c = _ratio(t["qpos"] - s["qpos"], ab.max() * h * h + 1e-5)
    expect(c <= 1.0, f"world {w}: qpos {c:.2f} of its bound")
    ssc = max(1.0, float(np.abs(s["sensordata"]).max()))
    c = _ratio(t["sensordata"] - s["sensordata"], 3e-3 * ssc)
    expect(c <= 1.0, f"world {w}: step sensordata {c:.2f} of its bound")
    R["sens"] = max(R["sens"], c)
    ni = int(t["solver_niter"].reshape(-1)[0])
    expect(abs(ni - s["niter"]) <= 1, f"world {w}: niter {ni} vs {s['niter']}")
  nefc = [s["nefc"] for s in step]
  print(f"{name}: nv {m.nv} nefc {min(nefc)}..{max(nefc)} fallback worlds {nfallback} ratios "
        + " ".join(f"{k} {v:.3f}" for k, v in R.items())
        + (" per-tree xpos err " + " ".join(f"{r}: {e:.2e}" for r, e in tree_err.items()) if len(trees) > 1 else ""))
  if len(trees) > 1:  # per tree, so that a tree left in its root's frame reads as such
    for r, e in tree_err.items():
      expect(e <= 2e-5, f"tree rooted at body {r}: xpos off by {e:.3e} (every tree's errors: {tree_err})")
  assert not bad, f"{name}: {len(bad)} mismatches, first: " + "; ".join(bad[:6])
  return R


@pytest.mark.parametrize("name", zoo.RUNNABLE)
def test_generic_kernels_match_the_oracle(name, generic):
  out = generic[name]
  assert out["info"][0] == 0 and out["info"][1] == 0, "specialize='never' ran a specialised kernel"
  assert (int(out["info"][2]), int(out["info"][3])) == (48, NJMAX)
  check_model(name, out)
  if zoo.get(name).props.get("rows64"):
    nefc = out["step_nefc"].reshape(-1)
    assert (nefc <= 64).sum() * 4 >= nefc.size and (nefc > 64).sum() * 4 >= nefc.size


@pytest.mark.parametrize("name", FUSED)
def test_four_substeps_equal_four_steps(name, generic):
  rep = json.loads(str(generic[name]["fused_bad"]))
  assert not rep["fields"], f"{name}: fused 4-substep step differs from 4 single steps: {rep}"


def test_specialised_model_matches_the_oracle(specialised):
  """The run-time specialised kernels (the first tree-form Cholesky on a dof tree that is not a
  robot's: a star with a three-joint body) loaded from the cache build() filled, in the fast and
  the maximum carve; against the oracle, not bit for bit against the generic run (the two
  families eliminate in different orders, tests/test_gpu_kernel_variants.py); and their
  four-substep step equals four single steps bit for bit."""
  out = specialised[SPECIALISED]
  assert out["info"][0] > 0 and out["info"][1] > 0, \
    f"{SPECIALISED} did not run its specialised kernels (spec ids {out['info'][:2]}): build() prebuilds them"
  check_model(SPECIALISED, out)
  rep = json.loads(str(out["fused_bad"]))
  assert not rep["fields"], f"specialised fused 4-substep step differs from 4 single steps: {rep}"
