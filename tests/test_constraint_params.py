"""The fp64 oracle's constraint parameters against an independent reference (CPU).

oracle/oracle.c and the engine's phase A were written from one reading of mj_contactParam and
mj_makeImpedance, and every engine test of these rules compares with that oracle.  Here the
oracle is held to tests/constraint_ref.py, a numpy restatement of the documented rules with an
exact active-set solver, on the probe scenes of tests/constraint_scenes.py: 7 scenes x 32
worlds, every world with its own geom / joint parameters (priority, condim, friction, solmix,
solref of both signs and below 2 h, every solimp shape, margin, gap, impratio; limit ranges,
margins, solref, solimp, both sides of a limit at once).

  ncon, nefc                               equal
  qacc, efc_force, contact force (frame)   1e-9 max(1, |value|)

Measured: 6e-14 relative at most.  Before in-gap contacts lost their rows (a contact with
margin - gap <= dist < margin stays in the contact list, mjContact.exclude = 1, without rows or
force), exactly the in-gap worlds failed here: nefc 1 or 4 against 0.

Mutant visibility: every rule of constraint_ref.MUTANTS, replaced by a plausible wrong one,
moves qacc in at least 4 worlds by more than 10 x the GPU test's qacc bound
(2e-3 max(1, max|qacc|), tests/test_gpu_constraint_params.py), so the sampled parameters and
states can tell the rules apart.
"""

from __future__ import annotations

import numpy as np
import pytest

import constraint_ref as cr
import constraint_scenes as cs

TOL = 1e-9
GPU_QACC_BOUND = 2e-3  # x max(1, max|qacc|): tests/test_gpu_parity.py
MUTANT_WORLDS, MUTANT_FACTOR = 4, 10.0


def _frame(name, w):
  """Any right-handed orthonormal frame on the exact normal (the mutant runs need no oracle)."""
  n = cs.ref_scene(name)["plane_normal"]
  t = np.cross(n, (0.0, 1.0, 0.0))
  t /= np.linalg.norm(t)
  return np.concatenate([n, t, np.cross(n, t)])


def _close(a, b):
  a, b = np.asarray(a, float), np.asarray(b, float)
  return a.shape == b.shape and bool(np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b))))


@pytest.mark.parametrize("name", cs.SCENES)
def test_oracle_matches_the_reference(name):
  bad, worst = [], 0.0
  for w in range(cs.NWORLD):
    o = cs.oracle_world(name, w)
    r = cs.reference(name, w, frame=o["frame"])
    assert r["nsets"] == 1  # solve_rows found exactly one consistent active set
    if (o["ncon"], o["nefc"]) != (r["ncon"], r["nefc"]):
      bad.append(f"world {w}: ncon / nefc {o['ncon']} / {o['nefc']} vs {r['ncon']} / {r['nefc']}")
      continue
    for k in ("qacc", "efc_force", "qfrc_constraint") + (("contact_force",) if name != "limit_pair" else ()):
      if np.size(r[k]):
        worst = max(worst, float(np.max(np.abs(o[k] - r[k]) / np.maximum(1.0, np.abs(r[k])))))
      if not _close(o[k], r[k]):
        bad.append(f"world {w}: {k} {o[k]} vs {r[k]}")
    if r["ncon"]:
      if not (_close(o["dist"], r["dist"]) and _close(o["pos"], r["pos"])):
        bad.append(f"world {w}: contact dist / pos {o['dist']} {o['pos']} vs {r['dist']} {r['pos']}")
  print(f"{name}: largest relative difference {worst:.1e}")
  assert not bad, f"{name}: {len(bad)} mismatches: " + "; ".join(bad[:8])


def test_states_keep_the_tie_clearance_and_cover_every_case():
  ingap = both = beyond = below2h = 0
  for name in cs.SCENES:
    f = cs.fields(name)
    q, _ = cs.states(name)
    for w in range(cs.NWORLD):
      if name == "limit_pair":
        n = 0
        for k in range(2):
          lo, hi = f["jnt_range"][w, k]
          for dist in (q[w, k] - lo, hi - q[w, k]):
            assert abs(dist - f["jnt_margin"][w, k]) >= cs.TIE_CLEARANCE, (name, w, k)
            n += dist < f["jnt_margin"][w, k]
          both += (q[w, k] - lo < f["jnt_margin"][w, k]) and (hi - q[w, k] < f["jnt_margin"][w, k])
        assert n == cs.reference(name, w)["nefc"]
      else:
        r = cs.reference(name, w, frame=_frame(name, w))
        p = r["params"]
        assert abs(r["dist"] - p["margin"]) >= cs.TIE_CLEARANCE, (name, w)
        assert abs(r["dist"] - p["includemargin"]) >= cs.TIE_CLEARANCE, (name, w)
        ingap += p["includemargin"] < r["dist"] < p["margin"]
        beyond += r["dist"] > p["margin"]
        below2h += 0 < p["solref"][0] < 2 * cs.H
  assert ingap >= 6 * 6 and beyond >= 6 * 6 and both >= 8 and below2h >= 6


def _applies(mutant, name):
  if mutant in cr.CONTACT_MUTANTS:
    return name != "limit_pair"
  if mutant in cr.LIMIT_MUTANTS:
    return name == "limit_pair"
  return True


@pytest.mark.parametrize("mutant", cr.MUTANTS)
def test_every_mutant_is_visible(mutant):
  """A rule that no world makes visible means the inputs are wrong (not the threshold)."""
  seen = 0
  for name in cs.SCENES:
    if not _applies(mutant, name):
      continue
    for w in range(cs.NWORLD):
      fr = None if name == "limit_pair" else _frame(name, w)
      true = cs.reference(name, w, frame=fr)
      mut = cs.reference(name, w, frame=fr, mutate=mutant)
      bound = GPU_QACC_BOUND * max(1.0, float(np.abs(true["qacc"]).max()))
      seen += bool(np.abs(mut["qacc"] - true["qacc"]).max() > MUTANT_FACTOR * bound)
  assert seen >= MUTANT_WORLDS, f"{mutant}: visible in {seen} worlds"


@pytest.mark.parametrize("name", ("params14", "params38"))
def test_zoo_parameter_models_put_contacts_in_their_gap_and_limits_on_both_sides(name):
  """The coupled problems the enumeration cannot reach run through the zoo's machinery
  (tests/test_model_zoo_cpu.py, tests/test_gpu_model_zoo.py); here, what their states must hold."""
  import model_zoo as zoo
  import oracle_lib as ol
  from oracle_sim import OracleData
  zm = zoo.get(name)
  m = zm.model
  assert len(set(np.asarray(m.arrays["geom_priority"]).tolist())) == 2
  assert set(np.asarray(m.arrays["geom_condim"]).tolist()) == {1, 3}
  assert (np.asarray(m.arrays["geom_solref"])[:, 0] < 0).any() and (np.asarray(m.arrays["geom_gap"]) > 0).all()
  lim = np.flatnonzero(np.asarray(m.jnt_limited))
  rng_, mg_ = np.asarray(m.arrays["jnt_range"])[lim], np.asarray(m.arrays["jnt_margin"])[lim]
  assert (mg_ > 0).all() and (rng_[:, 1] - rng_[:, 0] < 2 * mg_).any() and (rng_[:, 1] - rng_[:, 0] > 2 * mg_).any()
  q, qv, ctrl = zm.states()
  od = OracleData(m, 256, 1024)
  plane = int(np.flatnonzero(np.asarray(m.geom_type) == zoo.GEOM_PLANE)[0])
  ingap = both = 0
  for w in range(q.shape[0]):
    r = ol.forward(m, q[w], qv[w], None, ctrl[w], 0.0, step=False, nconmax=64, njmax=160)
    rows, gapped = 0, 0
    for c in r["contact"]:
      g = int(c[1]) if int(c[0]) == plane else int(c[0])
      _, margin, im = zoo.contact_thresholds(m, g)
      assert min(abs(c[2]), abs(c[2] - margin), abs(c[2] - im)) >= zoo.TIE_CLEARANCE, (name, w)
      gapped += im <= c[2] < margin
      if c[2] < im:
        pg, pp = int(m.arrays["geom_priority"][g]), int(m.arrays["geom_priority"][plane])
        dim = int(m.arrays["geom_condim"][g if pg > pp else plane]) if pg != pp else \
          max(int(m.arrays["geom_condim"][g]), int(m.arrays["geom_condim"][plane]))
        rows += 1 if dim == 1 else 4
    for _, g, z in zoo.surface_points(m, od, q[w]):
      assert all(abs(z - t) >= zoo.TIE_CLEARANCE for t in zoo.contact_thresholds(m, g)), (name, w)
    two = 0
    for _, lo, hi, mg in zoo.limit_distances(m, q[w]):
      assert abs(lo - mg) >= zoo.TIE_CLEARANCE and abs(hi - mg) >= zoo.TIE_CLEARANCE, (name, w)
      rows += (lo < mg) + (hi < mg)
      two += lo < mg and hi < mg
    assert rows == r["nefc"], (name, w, rows, r["nefc"])  # in-gap contacts have no rows
    ingap += gapped > 0
    both += two > 0
  assert ingap * 4 >= q.shape[0] and both * 4 >= q.shape[0], (ingap, both)
