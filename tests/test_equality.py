"""Joint equality constraints without a GPU: the compiler and Spec surface, the descriptor checks
of mjx_model_create, the row-capacity arithmetic, and the fp64 reference against itself.

The reference checks show that the inputs of tests/test_gpu_equality.py make every rule visible:
every mutant of equality_ref.MUTANTS moves some world's qacc by more than the GPU test's bound
there (the larger of 2e-3 max(1, max|qacc|) and 1e-4 + 1024 eps32 s_i), and the reference alone
meets each "at least a quarter of the worlds" condition of tests/equality_scenes.py.
"""

import copy
import ctypes

import numpy as np
import pytest

import equality_ref as er
import equality_scenes as es
from mjlab_amd.spec import Spec, mjtEq, mjtJoint

EPS32 = float(np.finfo(np.float32).eps)
SCALAR = ('<body name="a"><joint name="l" type="slide" axis="0 0 1"/><geom size="0.1" mass="1"/></body>'
          '<body name="b" pos="1 0 0"><joint name="r" type="hinge" axis="0 1 0" ref="0.1"/><geom size="0.1" mass="1"/></body>')
BODIES = (SCALAR + '<body name="c" pos="2 0 0"><joint name="ball" type="ball"/><geom size="0.1" mass="1"/></body>'
          '<body name="d" pos="3 0 0"><freejoint name="free"/><geom size="0.1" mass="1"/></body>')


def _xml(equality: str, default: str = "") -> str:
  return (f'<mujoco><compiler angle="radian"/>{default}<worldbody>{SCALAR}</worldbody>'
          f'<equality>{equality}</equality></mujoco>')


def _eq_arrays(m):
  return {k: np.asarray(v) for k, v in m.arrays.items() if k.startswith("eq_")}


# ----------------------------------------------------------------------------- compiler, Spec
def test_mjcf_and_add_equality_compile_to_the_same_arrays():
  a = Spec.from_string(_xml('<joint name="c" joint1="l" joint2="r" polycoef="0.02 -1 0.3" solref="0.01 0.8"'
                            ' solimp="0.8 0.9 0.01 0.4 3"/><joint joint1="r" polycoef="0.3" active="false"/>')).compile()
  s = Spec.from_string(_xml("").replace("<equality></equality>", ""))
  assert s.equalities == []
  e = s.add_equality(name="c", type=mjtEq.mjEQ_JOINT, name1="l", name2="r", data=[0.02, -1, 0.3],
                     solref=[0.01, 0.8], solimp=[0.8, 0.9, 0.01, 0.4, 3])
  s.add_equality(name1="r", data=[0.3], active=False)
  assert (e.name1, e.name2, s.equality("c").data.tolist()) == ("l", "r", [0.02, -1.0, 0.3, 0.0, 0.0])
  b = s.compile()
  ea, eb = _eq_arrays(a), _eq_arrays(b)
  assert set(ea) == set(eb) == {"eq_type", "eq_obj1id", "eq_obj2id", "eq_active0", "eq_data", "eq_solref", "eq_solimp"}
  for k in ea:
    assert ea[k].shape == eb[k].shape and np.array_equal(ea[k], eb[k]), k
  assert a.names["equality"] == b.names["equality"] == ["c", ""]
  assert a.neq == 2 and ea["eq_type"].tolist() == [2, 2]
  assert ea["eq_obj1id"].tolist() == [0, 1] and ea["eq_obj2id"].tolist() == [1, -1]
  assert ea["eq_active0"].tolist() == [1, 0]
  # fewer than five coefficients: the rest keep MuJoCo's defaults "0 1 0 0 0"
  assert ea["eq_data"].tolist() == [[0.02, -1.0, 0.3, 0.0, 0.0], [0.3, 1.0, 0.0, 0.0, 0.0]]
  assert ea["eq_solref"].tolist() == [[0.01, 0.8], [0.02, 1.0]]
  assert ea["eq_solimp"].tolist() == [[0.8, 0.9, 0.01, 0.4, 3.0], [0.9, 0.95, 0.001, 0.5, 2.0]]
  s.delete(s.equality("c"))
  assert [q.name1 for q in s.equalities] == ["r"] and s.compile().neq == 1


def test_defaults_and_default_classes_are_honoured():
  m = Spec.from_string(_xml('<joint joint1="l" joint2="r"/><joint class="soft" joint1="r"/>',
                            '<default><equality solref="0.03 0.7"/><default class="soft">'
                            '<equality solimp="0.5 0.6 0.01 0.5 2" polycoef="0.1 2"/></default></default>')).compile()
  e = _eq_arrays(m)
  assert e["eq_data"].tolist() == [[0.0, 1.0, 0.0, 0.0, 0.0], [0.1, 2.0, 0.0, 0.0, 0.0]]
  assert e["eq_solref"].tolist() == [[0.03, 0.7], [0.03, 0.7]]
  assert e["eq_solimp"].tolist() == [[0.9, 0.95, 0.001, 0.5, 2.0], [0.5, 0.6, 0.01, 0.5, 2.0]]
  assert e["eq_active0"].tolist() == [1, 1]


def test_attach_prefixes_the_joint_names():
  child = Spec.from_string(_xml('<joint name="c" joint1="l" joint2="r" polycoef="0 -1"/>'))
  parent = Spec()
  parent.worldbody.add_body(name="base").add_joint(name="j0", type=mjtJoint.mjJNT_HINGE)
  parent.body("base").add_geom(size=[0.1], mass=1.0)
  parent.attach(child, prefix="yam/")
  (e,) = parent.equalities
  assert (e.name, e.name1, e.name2) == ("yam/c", "yam/l", "yam/r")
  m = parent.compile()
  jn = m.names["joint"]
  assert m.names["equality"] == ["yam/c"]
  assert (jn[int(m.arrays["eq_obj1id"][0])], jn[int(m.arrays["eq_obj2id"][0])]) == ("yam/l", "yam/r")
  assert child.equalities[0].name1 == "l"  # the child is untouched


@pytest.mark.parametrize("kind", ["connect", "weld", "tendon", "flex", "distance"])
def test_other_equality_kinds_are_refused_by_name(kind):
  with pytest.raises(NotImplementedError, match=kind):
    Spec.from_string(_xml(f'<{kind} name="x" body1="a" body2="b"/>'))
  with pytest.raises(NotImplementedError, match=kind):
    Spec().add_equality(type=getattr(mjtEq, "mjEQ_" + kind.upper()), name1="a", name2="b")


@pytest.mark.parametrize("eq,words", [
    ('<joint joint1="l" joint2="ball"/>', "hinge or slide"), ('<joint joint1="free" joint2="l"/>', "hinge or slide"),
    ('<joint joint1="l" joint2="nope"/>', "no joint 'nope'"), ('<joint joint1="l" joint2="l"/>', "same joint")])
def test_bad_joints_are_value_errors(eq, words):
  xml = f'<mujoco><worldbody>{BODIES}</worldbody><equality>{eq}</equality></mujoco>'
  with pytest.raises(ValueError, match=words):
    Spec.from_string(xml).compile()


def test_a_model_without_equalities_has_no_eq_arrays():
  m = Spec.from_string(_xml("")).compile()
  assert m.neq == 0 and not _eq_arrays(m) and "equality" not in m.names
  from mjlab_amd._capi import make_desc
  desc, keep = make_desc(m)
  assert desc.neq == 0
  del keep


@pytest.mark.parametrize("task,asset", [("Mjlab-Velocity-Flat-Unitree-G1", "g1_velocity"),
                                        ("Mjlab-Velocity-Flat-Unitree-Go1", "go1_velocity")])
def test_shipped_scenes_compile_to_the_arrays_they_had(task, asset):
  from mjlab_amd.envs import load_env_cfg
  from mjlab_amd.scene import Scene
  from mjlab_amd.scenes import load_scene
  m, ref = Scene(load_env_cfg(task, False).scene, "cpu").compile(), load_scene(asset)
  assert m.names == ref.names and "equality" not in m.names
  assert list(m.arrays) == list(ref.arrays) and not _eq_arrays(m)
  for k in m.arrays:
    assert np.array_equal(np.asarray(m.arrays[k]), np.asarray(ref.arrays[k])), k


# ----------------------------------------------------------------------------- mjx_model_create
def _create_error(m, neq=None) -> bytes:
  """mjx_model_create's error through the real library (tests/test_model_tables.py): without a
  GPU an admitted descriptor fails at the first device call, with HIP's words."""
  from mjlab_amd._capi import make_desc
  from mjlab_amd._lib import lib
  desc, keep = make_desc(m)
  if neq is not None:
    desc.neq = neq
  ptr = ctypes.c_void_p()
  status = lib().mjx_model_create(ctypes.byref(desc), 0, ctypes.byref(ptr))
  del keep
  if status == 0:
    lib().mjx_model_destroy(ptr)
    return b""
  return lib().mjx_last_error()


def _edited(**arrays):
  m = copy.copy(es.model("lock"))
  m.arrays = {k: np.array(v) for k, v in m.arrays.items()}
  for k, v in arrays.items():
    m.arrays[k] = np.asarray(v, m.arrays[k].dtype)
  return m


def test_an_admitted_equality_model_passes_the_descriptor_checks():
  assert b"equality" not in _create_error(es.model("lock"))


@pytest.mark.parametrize("edit,words", [
    (dict(eq_type=[2, 1]), b"equality 1: only joint equalities are supported (eq_type 1)"),
    (dict(eq_obj1id=[2, 1]), b"equality 0: joint id out of range"),
    (dict(eq_obj2id=[-2, 0]), b"equality 0: joint id out of range"),
    (dict(eq_obj2id=[0, 0]), b"equality 0: joint1 and joint2 are the same joint"),
    (dict(jnt_type=[1, 2]), b"equality 0: a joint equality takes hinge or slide joints")])
def test_bad_descriptors_are_refused_before_device_work(edit, words):
  assert _create_error(_edited(**edit)) == words


def test_more_than_64_equalities_are_refused():
  m = _edited()
  for k in ("eq_type", "eq_obj1id", "eq_obj2id", "eq_active0", "eq_data", "eq_solref", "eq_solimp"):
    v = m.arrays[k]
    m.arrays[k] = np.concatenate([v[:1]] * 65)
  assert _create_error(m) == b"at most 64 equality constraints per world supported"
  for k in list(m.arrays):
    if k.startswith("eq_"):
      m.arrays[k] = m.arrays[k][:64]
  assert b"equality" not in _create_error(m)


# ----------------------------------------------------------------------------- capacities
def test_row_capacities_add_two_rows_per_equality():
  from mjlab_amd.sim import SimulationCfg
  from mjlab_amd.sim.sim import max_capacity, world_capacity
  m = es.model("gripper")
  bare = copy.copy(m)
  bare.arrays = {k: v for k, v in m.arrays.items() if not k.startswith("eq_")}
  nlim = int(np.sum(m.jnt_limited))
  assert nlim == 2 and m.neq == 1
  cfg = SimulationCfg(nconmax=48, njmax=None)
  assert max_capacity(cfg, bare)[1] == 4 * 64 + 2 * nlim
  assert max_capacity(cfg, m)[1] == 4 * 64 + 2 * nlim + 2
  cfg = SimulationCfg(engine_capacity=(1, 200))
  assert world_capacity(cfg, bare) == (1, 4 + 2 * nlim)
  assert world_capacity(cfg, m) == (1, 4 + 2 * nlim + 2)


def test_specialize_always_is_refused_for_an_equality_model():
  from mjlab_amd.sim import Simulation, SimulationCfg
  with pytest.raises(NotImplementedError, match="equality"):
    Simulation(1, SimulationCfg(specialize="always"), copy.deepcopy(es.model("lock")), "cuda:0")


# ----------------------------------------------------------------------------- the reference
def _rows(name, w):
  r = es.reference(name, w)
  k = r["always"]
  return r, (r["J"][k], r["D"][k], r["aref"][k]), (r["J"][~k], r["D"][~k], r["aref"][~k])


@pytest.mark.parametrize("name", ["slide_pair", "quartic", "lock", "gripper"])
def test_an_always_active_row_and_the_opposed_pair_agree(name):
  worst, kkt = 0.0, 0.0
  for w in range(es.NWORLD):
    r, eq, ineq = _rows(name, w)
    a0 = np.linalg.solve(r["M"], r["qfrc_smooth"])
    one = er.solve(r["M"], a0, *eq, *ineq)
    two = er.solve(r["M"], a0, *eq, *ineq, pair=True)
    sc = max(1.0, float(np.abs(one["qacc"]).max()))
    worst = max(worst, float(np.abs(one["qacc"] - two["qacc"]).max()) / sc)
    # at most one row of each pair carries force, and it carries the equality's
    ne = eq[0].shape[0]
    f2 = two["f_moved"]
    assert np.all(np.minimum(f2[:ne], f2[ne:]) == 0.0)
    assert np.allclose(f2[:ne] - f2[ne:], one["f_eq"], rtol=1e-9, atol=1e-9 * sc)
    assert np.allclose(one["qacc"], r["qacc"], rtol=0, atol=1e-9 * sc)
    kkt = max(kkt, one["kkt"] / max(1.0, float(np.abs(r["M"] @ one["qacc"]).max())), two["kkt"])
  print(f"{name}: pair vs always-active {worst:.2e}, KKT residual {kkt:.2e}")
  assert worst <= 1e-12
  assert kkt <= 1e-10  # rounding of the dual solve: ~1e3 ulps of the terms


def test_the_generic_reference_agrees_with_the_closed_form_on_slide_pair():
  m = es.model("slide_pair")
  p = es.PAIR
  assert np.allclose(m.arrays["dof_invweight0"], [1 / (p["m1"] + p["arm1"]), 1 / (p["m2"] + p["arm2"])], rtol=1e-12)
  q, qv, ctrl = es.states("slide_pair")
  for w in range(es.NWORLD):
    g, c = es.generic_reference(m, q[w], qv[w], ctrl[w]), es.reference("slide_pair", w)
    sc = max(1.0, float(np.abs(c["qacc"]).max()))
    assert np.abs(g["qacc"] - c["qacc"]).max() <= 1e-10 * sc
    assert np.abs(g["qvel"] - c["qvel"]).max() <= 1e-12 * sc and np.abs(g["qpos"] - c["qpos"]).max() <= 1e-13
    assert g["nefc"] == c["nefc"] == 2


def _gpu_bound(name, w, r):
  sc = max(1.0, float(np.abs(r["qacc"]).max()))
  return np.maximum(2e-3 * sc, 1e-4 + 1024.0 * EPS32 * es.qacc_scale(name, w))


@pytest.mark.parametrize("mutant", er.MUTANTS)
def test_every_mutant_moves_some_world_past_the_gpu_bound(mutant):
  seen = {}
  for name in ("slide_pair", "quartic", "lock", "gripper", "mixed"):
    for w in range(es.NWORLD):
      r = es.reference(name, w)
      x = es.reference(name, w, mutate=mutant)
      ratio = float(np.max(np.abs(x["qacc"] - r["qacc"]) / _gpu_bound(name, w, r)))
      seen[name] = max(seen.get(name, 0.0), ratio)
  print(mutant, {k: round(v, 1) for k, v in seen.items()})
  assert max(seen.values()) > 1.0, f"{mutant} is invisible on every scene: {seen}"


def test_the_scenes_meet_their_quarter_conditions():
  n = es.NWORLD
  f = es.fields("quartic")
  assert sum(1 for w in range(n) if f["eq_solref"][w, 0, 0] < 0) * 4 >= n
  assert len({tuple(f[k][w].reshape(-1)) for k in es.EQ_FIELDS for w in range(n)}) == 3 * n
  x = np.array([abs(es.reference("quartic", w)["eq_pos"][0]) / f["eq_solimp"][w, 0, 2] for w in range(n)])
  assert (x == 0).any() and ((x > 0.05) & (x < 0.5)).sum() >= 5 and ((x > 0.5) & (x < 1)).sum() >= 5 and (x > 1).any()
  assert all(es.reference("lock", w)["nefc"] == 2 for w in range(n))
  assert sum(1 for w in range(n) if es.reference("gripper", w)["nlim"] > 0) * 4 >= n
  assert sum(1 for w in range(n) if es.reference("mixed_many", w)["nefc"] > 64) * 4 >= n
  mixed = [es.reference("mixed", w) for w in range(n)]
  assert sum(1 for r in mixed if r["nlim"] > 0 and r["ncrow"] == 4) * 4 >= n
  assert {r["ncrow"] for r in mixed} == {0, 4} and {r["nlim"] for r in mixed} >= {1, 2}
