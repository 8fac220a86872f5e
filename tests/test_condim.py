"""Torsional and rolling friction (condim 4 and 6) without a GPU: the compiled fields of the
probe scenes, the refusal of other contact dimensions, the row-capacity arithmetic, the
descriptor field, and the fp64 reference against itself.

The reference checks show that the inputs of tests/test_gpu_condim.py make every rule visible:
every mutant of condim_ref.MUTANTS moves some world's qacc, contact_force or contact_torque by
more than the GPU test's bound there (qacc: 2e-3 max(1, max|qacc|); the wrench: condim_scenes.
force_bounds with that qacc bound), and on a condim-3 world the reference is constraint_ref's.
"""

import copy
import ctypes

import numpy as np
import pytest

import condim_ref as ref
import condim_scenes as sc
import constraint_ref as cr
import constraint_scenes as cs
from mjlab_amd.spec import Spec


# ----------------------------------------------------------------------------- compiled fields
@pytest.mark.parametrize("name", sc.SCENES)
def test_compiled_fields_of_the_scenes(name):
  m = sc.model(name)
  assert m.max_condim == sc.MAX_CONDIM[name] == int(np.max(m.arrays["geom_condim"]))
  f = sc.fields(name)["geom_friction"]
  assert f.shape == (sc.NWORLD, m.ngeom, 3)
  # three distinct components in every world, and the model's own friction as compiled
  assert np.all(f[:, :, 0] != f[:, :, 1]) and np.all(f[:, :, 1] != f[:, :, 2])
  assert np.asarray(m.arrays["geom_friction"]).shape == (m.ngeom, 3)
  binv = np.asarray(m.arrays["body_invweight0"], float)
  free = {"spin_plane4": [("ball", sc.BALL)], "spin_plane6": [("ball", sc.BALL)],
          "two_balls6": [("ball", sc.BALL), ("ballb", sc.BALL_B)], "many70": [("plate", sc.PLATE)]}
  for bname, b in free.get(name, []):
    k = m.names["body"].index(bname)
    np.testing.assert_allclose(binv[k], [1.0 / b["mass"], np.mean(1.0 / np.asarray(b["inertia"]))], rtol=1e-12)
  if name == "hinge_pad6":
    b = sc.world_geometry(name, 0)[0][0]
    np.testing.assert_allclose(binv[m.names["body"].index("arm")], [b.tran, b.rot], rtol=1e-12)
  if name == "many70":
    cd = np.asarray(m.arrays["geom_condim"])
    assert m.ngeom == 71 and int(np.sum(cd == 6)) == 4 and int(np.sum(cd == 1)) == 67


def test_models_without_such_geoms_have_max_condim_3():
  for k in range(len(cs.BALL_MODELS)):
    assert cs.model(f"ball_plane{k}").max_condim == 3
  assert cs.model("limit_pair").max_condim == 3


@pytest.mark.parametrize("condim", [2, 5, 0, 7])
def test_other_contact_dimensions_are_value_errors(condim):
  with pytest.raises(ValueError, match=f"geom 'ball': condim {condim} is not supported"):
    sc.compile_xml(sc.scene_xml("spin_plane6", condim=condim))
  # through Spec's own geoms
  s = Spec.from_string(sc.scene_xml("spin_plane6"))
  s.geom("ball").condim = condim
  with pytest.raises(ValueError, match=f"geom 'ball': condim {condim}"):
    s.compile()


def test_a_collision_edit_condim_is_checked():
  from mjlab_amd.compiler.model import CollisionEdit, EntitySpec, compile_scene
  from mjlab_amd.compiler.mjcf import parse_mjcf_string
  xml = parse_mjcf_string(sc.scene_xml("spin_plane6"))
  ok = compile_scene([EntitySpec(name="", xml=xml, collisions=(CollisionEdit(geom_names_expr=("ball",), condim=4),))],
                     terrain="none")
  assert ok.max_condim == 4
  with pytest.raises(ValueError, match="condim 5 is not supported"):
    compile_scene([EntitySpec(name="", xml=xml, collisions=(CollisionEdit(geom_names_expr=("ball",), condim=5),))],
                  terrain="none")


# ----------------------------------------------------------------------------- capacities
def test_capacities_of_condim_4_and_6_models():
  from mjlab_amd.sim import SimulationCfg
  from mjlab_amd.sim.sim import max_capacity, world_capacity
  m4, m6 = sc.model("spin_plane4"), sc.model("spin_plane6")
  cfg = SimulationCfg(nconmax=48, njmax=None)
  assert max_capacity(cfg, m4) == (6 * 64, 6 * 64)
  assert max_capacity(cfg, m6) == (512, 10 * 64)
  assert world_capacity(cfg, m4) == (48, 160) and world_capacity(cfg, m6) == (48, 160)
  cfg = SimulationCfg(engine_capacity=(2, 200))
  assert world_capacity(cfg, m4) == (2, 12) and world_capacity(cfg, m6) == (2, 20)
  assert world_capacity(cfg, cs.model("ball_plane2")) == (2, 8)


def _capacities(m):
  from mjlab_amd.sim import SimulationCfg
  from mjlab_amd.sim.sim import max_capacity, world_capacity
  out = []
  for cfg in (SimulationCfg(nconmax=48, njmax=None), SimulationCfg(nconmax=None, njmax=300),
              SimulationCfg(engine_capacity=(3, 200)), SimulationCfg(engine_capacity=(24, 96))):
    out += [world_capacity(cfg, m), max_capacity(cfg, m)]
  return out


def _parent_capacities(m):
  """The arithmetic before torsional / rolling contacts: four rows per contact."""
  nlim = int(np.sum(m.jnt_limited)) if m.njnt else 0
  neq = int(len(m.arrays.get("eq_type", ())))
  out = []
  for nconmax, njmax, ec in ((48, None, None), (None, 300, None), (None, None, (3, 200)), (None, None, (24, 96))):
    if ec is not None:
      ncon, cap = ec
    else:
      ncon, cap = int(min(64, max(nconmax if nconmax is not None else 48, 48))), 160
    rows = int(max(1, min(njmax if njmax is not None else cap, 4 * ncon + 2 * nlim + 2 * neq, cap)))
    rmax = max(rows, int(njmax) if njmax is not None else 4 * 64 + 2 * nlim + 2 * neq)
    out += [(ncon, rows), (max(ncon, min(rmax, 512)), rmax)]
  return out


@pytest.mark.parametrize("asset", ["g1_velocity", "go1_velocity"])
def test_capacities_of_the_shipped_scenes_are_unchanged(asset):
  from mjlab_amd.scenes import load_scene
  m = load_scene(asset)
  assert m.max_condim == 3
  assert _capacities(m) == _parent_capacities(m)


@pytest.mark.parametrize("name", cs.SCENES)
def test_capacities_of_the_constraint_scenes_are_unchanged(name):
  m = cs.model(name)
  assert _capacities(m) == _parent_capacities(m)


# ----------------------------------------------------------------------------- descriptor, sim
def test_descriptor_field_round_trips():
  from mjlab_amd._capi import ModelDesc, make_desc
  assert ModelDesc._fields_[-1][0] == "max_condim"  # appended behind the equality block
  for name, want in (("spin_plane4", 4), ("many70", 6)):
    desc, keep = make_desc(sc.model(name))
    assert desc.max_condim == want
    del keep
  desc, keep = make_desc(cs.model("ball_plane2"))
  assert desc.max_condim == 3
  del keep


def _create_error(m, max_condim=None) -> bytes:
  """mjx_model_create's error through the real library (tests/test_model_tables.py): without a
  GPU an admitted descriptor fails at the first device call, with HIP's words."""
  from mjlab_amd._capi import make_desc
  from mjlab_amd._lib import lib
  desc, keep = make_desc(m)
  if max_condim is not None:
    desc.max_condim = max_condim
  ptr = ctypes.c_void_p()
  status = lib().mjx_model_create(ctypes.byref(desc), 0, ctypes.byref(ptr))
  del keep
  if status == 0:
    lib().mjx_model_destroy(ptr)
    return b""
  return lib().mjx_last_error()


def test_model_create_checks_the_contact_dimensions():
  m = sc.model("spin_plane6")
  assert b"condim" not in _create_error(m) and b"condim" not in _create_error(m, max_condim=0)
  assert _create_error(m, max_condim=4) == b"max_condim 4 is not the largest geom_condim (6)"
  bad = copy.copy(m)
  bad.arrays = dict(m.arrays)
  bad.arrays["geom_condim"] = np.array([3, 5], np.int32)
  assert _create_error(bad, max_condim=0) == b"geom 1: condim 5 is not supported (1, 3, 4 or 6)"


def test_specialize_always_is_refused_for_a_condim_6_model():
  from mjlab_amd.sim import Simulation, SimulationCfg
  with pytest.raises(NotImplementedError, match="torsional or rolling"):
    Simulation(1, SimulationCfg(specialize="always"), copy.deepcopy(sc.model("spin_plane6")), "cuda:0")


def test_jit_does_not_specialise_a_condim_6_model():
  from mjlab_amd import jit
  assert jit.ensure_library(sc.model("spin_plane6"), 48, 160, 0, compile_ok=True) is None


# ----------------------------------------------------------------------------- the reference
def _visible(name, w, mutate):
  """Does the mutant move world w's qacc or wrench past the GPU test's bounds?"""
  r, x = sc.reference(name, w), sc.reference(name, w, mutate=mutate)
  if r["nefc"] == 0:
    return False
  ab = np.full(r["qacc"].size, 2e-3 * max(1.0, float(np.abs(r["qacc"]).max())))
  if np.any(np.abs(x["qacc"] - r["qacc"]) > ab):
    return True
  b = sc.force_bounds(r, ab)
  for key, what in (("force", "contact_force"), ("torque", "contact_torque")):
    bound = b[key][0] + sc.FORCE_C * sc.EPS32 * b[key][1]
    if np.any(np.abs(x[what] - r[what]) > bound):
      return True
  return False


@pytest.mark.parametrize("mutate", ref.MUTANTS)
def test_every_mutant_is_visible_on_some_world(mutate):
  seen = [(name, w) for name in sc.REF_SCENES for w in range(sc.NWORLD) if _visible(name, w, mutate)]
  assert seen, f"{mutate}: no world of any scene shows it"
  if mutate in ("rot_rows_body2_only", "rot_sign_body1_kept"):
    assert {n for n, _ in seen} == {"two_balls6"}  # the only scene whose body 1 moves


def test_the_reference_has_one_active_set_and_the_expected_rows():
  for name in sc.REF_SCENES:
    rows = {sc.reference(name, w)["nefc"] for w in range(sc.NWORLD)}
    assert rows == {0, 2 * (sc.MAX_CONDIM[name] - 1)}, (name, rows)
    for w in range(sc.NWORLD):
      r = sc.reference(name, w)
      assert r["nsets"] == 1
      assert np.allclose(r["M"] @ (r["qacc"] - r["a0"]), r["qfrc_constraint"], rtol=1e-9, atol=1e-9)


def test_the_reference_reduces_to_constraint_ref_on_a_condim_3_world():
  name = "ball_plane2"  # plane and ball condim 3, impratio 4
  q, qv = cs.states(name)
  done = 0
  for w in range(cs.NWORLD):
    plane, ball = cs.ref_params(name, w)
    s = cs.ref_scene(name)
    frame = sc.any_frame(np.asarray(s["plane_normal"], float))
    want = cr.ball_plane(s, plane, ball, q[w], qv[w], frame=frame)
    b = ref.free_body(s["mass"], s["inertia"], q[w], 0, 6)
    dist = float(s["plane_normal"] @ b.c) - s["radius"]
    got = ref.contact_world(s["h"], s["impratio"], s["gravity"], [b], qv[w], plane, ball, None, b, dist,
                            b.c - s["plane_normal"] * (s["radius"] + 0.5 * dist), s["plane_normal"], frame=frame)
    assert (got["ncon"], got["nefc"]) == (want["ncon"], want["nefc"])
    for k in ("qacc", "efc_force", "qfrc_constraint", "contact_force"):
      np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=1e-12, err_msg=f"world {w} {k}")
    assert np.all(got["contact_torque"] == 0.0)
    qn, vn = ref.integrate_free(q[w], qv[w], got["qacc"], s["h"])
    np.testing.assert_allclose(qn, want["qpos"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(vn, want["qvel"], rtol=1e-12, atol=1e-12)
    done += want["nefc"] == 4
  assert done >= 8


def test_the_reference_spins_down_by_step_150():
  """The rollout of tests/test_gpu_condim.py, the reference alone: torsional friction stops the
  condim-4 ball well before step 150, and nothing slows the condim-3 ball."""
  om4, sets, _ = sc.spin_down_reference("spin_down4")
  om3, _, _ = sc.spin_down_reference("spin_down3")
  assert abs(om4[149]) < 0.05 * sc.SPIN_OMEGA and abs(om4[-1]) < 0.05 * sc.SPIN_OMEGA
  assert om4[0] < sc.SPIN_OMEGA and all(len(s) in (0, 6) for s in sets)
  np.testing.assert_allclose(om3, sc.SPIN_OMEGA, rtol=1e-12)
