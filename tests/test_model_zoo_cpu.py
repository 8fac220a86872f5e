"""The synthetic model zoo (tests/model_zoo.py) on the CPU: what each model claims, that the
zoo covers every generic register-row length of the engine, the fp64 oracle pinned on these
body trees by routes that share none of its formulas, and the contact populations the GPU
tests (tests/test_gpu_model_zoo.py) rely on.

Oracle pins (tests/invariants.py), at the tolerances of tests/test_oracle_invariants.py:
  - 1/2 v'Mv against the bodies' finite-difference twists, rel 1e-8 (measured <= 6.4e-11);
  - qfrc_bias against Lagrange's equations on a contact-free copy, rtol 1e-6 and atol 1e-6 of
    the largest entry on fixed-base trees (measured <= 1.3e-9 of it), rel / abs 1e-5 per dof on
    trees with a free joint (measured <= 1.5e-9 absolute), for every dof that is a true coordinate;
  - the rate of linear and of angular momentum about the com of the gravity-free multi-tree
    model, zero within 1e-5 of (total mass x the largest acceleration) (measured 1.3e-9).

Contact models are the trees with a free root: their states are dropped onto the plane.  A
fixed-base tree hangs from a base 1.2 to 1.5 m up and reaches at most 0.9 m down; its geoms
collide with the plane (the pairs exist) but never touch it, so the "half of the worlds touch"
condition does not apply to it, while the overflow and tie conditions do.

What the engine cannot compute it must refuse: the models of zoo.REJECTED (more than 60 dofs; a
tree that follows a tree of several bodies) fail mjx_model_create with those words, every other
zoo model and every shipped scene passes those checks, and ball joints, more than 64 bodies
and more than 64 dofs stay refused.
"""

import ctypes
import os
import re

import numpy as np
import pytest

import invariants as inv
import model_zoo as zoo
from oracle_sim import OracleData

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = os.path.join(ROOT, "mjlab-1_amd", "csrc", "engine.hip")
PIN_MODELS = ("multitree", "multitree_arm", "slide13", "star48", "chain24", "robot_object")
# dof counts the zoo must hold: the smallest and the largest that select each row length no
# robot runs, and every residue mod 4 above 36
REQUIRED_NV = (12, 13, 16, 21, 24, 29, 32, 37, 40, 45, 48, 53, 56, 61, 64)
FAST_ROWS, FAST_CONTACTS = 160, 48


def _children(m):
  return np.diff(np.asarray(m.arrays["body_childadr"]))


# ----------------------------------------------------------------------------- properties
@pytest.mark.parametrize("name", zoo.NAMES)
def test_properties(name):
  zm = zoo.get(name)
  m, p = zm.model, zm.props
  assert m.nv == p["nv"]
  assert m.nbody <= 64 and m.nv <= 64 and m.njnt <= 64 and m.nu <= 64
  types = np.asarray(m.jnt_type)
  assert set(types.tolist()) <= {zoo.JNT_FREE, zoo.JNT_SLIDE, zoo.JNT_HINGE}
  assert m.nu >= 1 and m.nsensordata >= 3
  assert (np.asarray(m.arrays["jnt_stiffness"]) > 0).any() or m.nv < 8
  assert np.asarray(m.jnt_limited).any() or m.nv < 9
  assert (np.asarray(m.dof_armature) > 0).any() and (np.asarray(m.arrays["dof_damping"]) > 0).any()
  gt = np.asarray(m.geom_type)
  assert set(gt.tolist()) <= {zoo.GEOM_PLANE, zoo.GEOM_SPHERE, zoo.GEOM_CAPSULE} and (gt == zoo.GEOM_PLANE).sum() == 1
  # collisions: every pair is the plane against a body geom
  plane = int(np.flatnonzero(gt == zoo.GEOM_PLANE)[0])
  assert m.npair > 0 and all(plane in (int(a), int(b)) for a, b in zip(m.arrays["pair_geom1"], m.arrays["pair_geom2"]))
  # non-identity body frames
  assert (np.abs(np.asarray(m.arrays["body_quat"])[2:, 0]) < 0.9999).any() or m.nbody <= 3
  level_body = np.asarray(m.arrays["level_body"])
  nlev = len(m.arrays["level_start"]) - 1
  ch, jn = _children(m), np.asarray(m.arrays["body_jntnum"])
  roots = np.asarray(m.body_rootid)
  if "nbody" in p:
    assert m.nbody == p["nbody"]
  if "levels" in p:
    assert nlev == p["levels"] >= 25 and (level_body == np.arange(m.nbody)).all()
    assert {zoo.JNT_SLIDE, zoo.JNT_HINGE} == set(types.tolist())
  if "max_joints" in p:
    assert jn.max() == p["max_joints"]
  if p.get("max_joints") == 3:
    b = int(np.argmax(jn))
    j0 = int(m.arrays["body_jntadr"][b])
    assert types[j0:j0 + 3].tolist() == [zoo.JNT_HINGE, zoo.JNT_HINGE, zoo.JNT_SLIDE]
  if "max_children" in p:
    assert ch[1:].max() == p["max_children"]
    assert set(p["child_counts"]) <= set(ch[1:].tolist())
  if p.get("slide_heavy"):
    assert (types == zoo.JNT_SLIDE).sum() > m.njnt // 2
  if p.get("star"):
    assert ch[1:].max() >= 6 and nlev <= 5
  if p.get("multitree"):
    # level order differs from body order: a later tree's root sits in a lane below its id
    assert not (level_body == np.arange(m.nbody)).all()
    tree = [int(r) for r in np.unique(roots[1:])]
    assert len(tree) == p["trees"]
    sizes = [(roots == r).sum() for r in tree]
    assert sizes[0] >= 8 and sizes[1] >= 8
    lane = {int(b): i for i, b in enumerate(level_body)}
    assert lane[tree[1]] != tree[1], "the second root's lane equals its id: the case is not exercised"
    free_roots = [r for r in tree if types[int(m.arrays["body_jntadr"][r])] == zoo.JNT_FREE]
    assert len(free_roots) == 2 and (len(tree) == 2 or p["trees"] == 3)
    q0 = np.asarray(m.qpos0)
    a = [int(m.jnt_qposadr[int(m.arrays["body_jntadr"][r])]) for r in free_roots]
    assert np.linalg.norm(q0[a[0]:a[0] + 3] - q0[a[1]:a[1] + 3]) > 1.0
  if p.get("robot_object"):
    last = m.nbody - 1
    assert roots[last] == last and ch[last] == 0 and (roots == roots[1]).sum() >= 8
    assert types[int(m.arrays["body_jntadr"][last])] == zoo.JNT_FREE
  if p.get("fixed"):
    assert (types != zoo.JNT_FREE).all()


def test_states_are_deterministic_and_near_the_origin():
  for name in ("multitree", "wave64"):
    zm = zoo.get(name)
    a, b = zm.states(4), zm.states(4)
    for x, y in zip(a, b):
      assert np.array_equal(x, y)
  for name in zoo.NAMES:
    zm = zoo.get(name)
    q, _, _ = zm.states(4)
    od = OracleData(zm.model)
    for w in range(4):
      x, _ = inv.body_pose(od, q[w])
      assert np.abs(x).max() < 3.0, name


# ----------------------------------------------------------------------------- row lengths
def _engine_row_lengths():
  text = open(ENGINE).read()
  line = re.search(r"#define MJX_GENERIC_NRS\(X\)(.*)", text).group(1)
  nrs = [int(v) for v in re.findall(r"X\((\d+)\)", line)]
  body = text[text.index("static StepFn generic_fn(int nv, int ph)"):]
  body = body[:body.index("\n}")]
  thresholds = [(int(a), int(b)) for a, b in re.findall(r"if \(nvp <= (\d+)\) return generic_fn_(\d+)\(ph\);", body)]
  last = int(re.search(r"\n\s*return generic_fn_(\d+)\(ph\);", body).group(1))
  return nrs, thresholds, last


def test_every_generic_row_length_has_a_model():
  nrs, thresholds, last = _engine_row_lengths()
  assert len(nrs) >= 10 and sorted(nrs) == nrs
  # the selection is "the smallest row length that holds the padded dof count"
  assert [t for t, _ in thresholds] == [n for _, n in thresholds] == nrs[:-1] and last == nrs[-1] == 64

  def selected(nv):
    nvp = (nv + 3) & ~3
    return next((n for t, n in thresholds if nvp <= t), last)

  # only the models the engine admits count: a refused model launches nothing
  have = {}
  for name in zoo.RUNNABLE:
    nv = zoo.get(name).model.nv
    assert selected(nv) == zoo.nr_for_nv(nv, nrs)
    have.setdefault(selected(nv), []).append(nv)
  assert sorted(have) == nrs, f"row lengths without a zoo model: {sorted(set(nrs) - set(have))}"
  assert set(REQUIRED_NV) <= {zoo.get(n).model.nv for n in zoo.NAMES}
  nvs = {zoo.get(n).model.nv for n in zoo.RUNNABLE}
  assert set(REQUIRED_NV) - nvs == {61, 64}, "only the dof counts past the engine's 60 may lack a running model"
  assert {nv % 4 for nv in nvs if nv > 36} == {0, 1, 2, 3}
  # every row length no robot runs: a model that fills it, and one that pads it by three lanes
  # (row length 64 up to the 60 dofs the engine admits: 60 pads by four lanes, 57 by seven)
  for n in nrs:
    if n not in (8, 20, 36):
      top = min(n, 60)
      assert top in nvs and top - 3 in nvs, f"row length {n}: no model with {top} and {top - 3} dofs"


# ----------------------------------------------------------------------------- oracle pins
def _pin_state(zm, w=1):
  q, qv, _ = zm.states(4)
  return q[w], 2.0 * qv[w]


@pytest.mark.parametrize("name", PIN_MODELS)
def test_kinetic_energy_from_body_twists(name):
  zm = zoo.get(name)
  m = inv.free_floating(zm.model)
  od = OracleData(m)
  q, v = _pin_state(zm)
  M = inv.mass_matrix(od, q)
  _, R = inv.body_pose(od, q)
  vb, wb = inv.fd_twists(od, q, v)
  ke = inv.kinetic_energy_bodies(m, R, vb, wb, v)
  print(f"{name}: KE rel err {abs(0.5 * v @ M @ v - ke) / ke:.2e}")
  assert 0.5 * v @ M @ v == pytest.approx(ke, rel=1e-8)
  od.qpos[:], od.qvel[:] = q, v
  od.forward()
  vc, wc = inv.twists_from_cvel(m, od.xipos, od.subtree_com, od.cvel)
  np.testing.assert_allclose(vc[1:], vb[1:], atol=1e-7)
  np.testing.assert_allclose(wc[1:], wb[1:], atol=1e-7)


@pytest.mark.parametrize("name", PIN_MODELS)
def test_bias_forces_from_lagrange(name):
  """qfrc_bias against d/dt(M) v - dT/dq + dU/dq on every dof with a true coordinate (a free
  joint's rotational dofs are quasi-velocities), on a contact-free copy."""
  zm = zoo.get(name)
  m = inv.free_floating(zm.model)
  od = OracleData(m)
  q, v = _pin_state(zm)
  od.qpos[:], od.qvel[:] = q, v
  od.forward()
  bias = od.qfrc_bias.copy()
  rows, has_free = [], False
  for j in range(m.njnt):
    d = int(m.jnt_dofadr[j])
    if int(m.jnt_type[j]) == zoo.JNT_FREE:
      rows += [d, d + 1, d + 2]
      has_free = True
    else:
      rows.append(d)
  lag = inv.lagrange_bias(od, q, v, rows)
  want = np.array([lag[i] for i in rows])
  err = np.abs(bias[rows] - want)
  print(f"{name}: Lagrange max err {err.max():.2e} of {np.abs(want).max():.2e}")
  if has_free:
    for k, i in enumerate(rows):
      assert bias[i] == pytest.approx(want[k], rel=1e-5, abs=1e-5 * max(1.0, abs(want[k]))), f"dof {i}"
  else:
    np.testing.assert_allclose(bias[rows], want, rtol=1e-6, atol=1e-6 * max(1.0, np.abs(want).max()))


def _momenta_at(od, q, v):
  m = od.model
  od.qpos[:], od.qvel[:] = q, v
  od.forward()
  vb, wb = inv.twists_from_cvel(m, od.xipos, od.subtree_com, od.cvel)
  return inv.momenta(m, od.xipos, od.ximat.reshape(-1, 3, 3), vb, wb)


def test_momentum_rate_gravity_free_multitree():
  """Two free-floating trees without gravity, contacts, springs or dampers: the oracle's
  forward dynamics must keep the linear momentum and the angular momentum about the com."""
  zm = zoo.get("multitree")
  m = zoo.gravity_free(zm)
  od = OracleData(m)
  q, v = _pin_state(zm)
  od.qpos[:], od.qvel[:] = q, v
  od.forward()
  a = od.qacc.copy()
  e = 1e-4
  Mt, _, Pp, Lp = _momenta_at(od, inv.integrate_pos(m, q, e * v + 0.5 * e * e * a, 1.0), v + e * a)
  _, _, Pm, Lm = _momenta_at(od, inv.integrate_pos(m, q, -e * v + 0.5 * e * e * a, 1.0), v - e * a)
  dP, dL = (Pp - Pm) / (2 * e), (Lp - Lm) / (2 * e)
  scale = Mt * max(1.0, float(np.abs(a).max()))
  print(f"momentum rates {np.abs(dP).max() / scale:.2e} {np.abs(dL).max() / scale:.2e} of the scale")
  np.testing.assert_allclose(dP, 0.0, atol=1e-5 * scale)
  np.testing.assert_allclose(dL, 0.0, atol=1e-5 * scale)


# ----------------------------------------------------------------------------- contacts
@pytest.fixture(scope="module")
def populations():
  import oracle_lib as ol
  out = {}
  for name in zoo.NAMES:
    zm = zoo.get(name)
    q, qv, ctrl = zm.states()
    out[name] = [ol.forward(zm.model, q[w], qv[w], None, ctrl[w], 0.0, step=False, nconmax=64, njmax=FAST_ROWS)
                 for w in range(q.shape[0])]
  return out


@pytest.mark.parametrize("name", zoo.NAMES)
def test_contact_population(name, populations):
  zm, refs = zoo.get(name), populations[name]
  ncon = np.array([r["ncon"] for r in refs])
  nefc = np.array([r["nefc"] for r in refs])
  print(f"{name}: ncon {ncon.min()}..{ncon.max()} nefc {nefc.min()}..{nefc.max()}")
  assert not any(r["overflow"] for r in refs)
  assert ncon.max() <= FAST_CONTACTS and nefc.max() <= FAST_ROWS
  assert len(refs) == zm.nworld
  if not zm.props.get("fixed"):  # (module docstring: a fixed-base tree hangs clear of the plane)
    assert (ncon > 0).sum() * 2 >= len(refs), "fewer than half of the worlds touch the plane"
  # no contact within 1e-4 of its activation distance (fp32 against fp64 must agree on ncon),
  # and no colliding geom within 1e-4 of touching in a world
  od = OracleData(zm.model)
  q, _, _ = zm.states()
  for w, r in enumerate(refs):
    assert all(abs(c[2]) > 1e-4 for c in r["contact"]), (name, w)
    if ncon[w] == 0:
      low = zoo.lowest_points(zm.model, od, q[w])
      assert all(abs(z) > 1e-4 for z in low.values()), (name, w)
  if zm.props.get("rows64"):
    assert (nefc <= 64).sum() * 4 >= len(refs) and (nefc > 64).sum() * 4 >= len(refs), nefc


# ----------------------------------------------------------------------------- rejections
def test_ball_joints_are_rejected():
  from mjlab_amd.spec import Spec
  xml = """<mujoco><worldbody><body pos="0 0 1"><joint type="ball"/>
           <geom type="sphere" size="0.1" mass="1"/></body></worldbody></mujoco>"""
  with pytest.raises(NotImplementedError):
    Spec.from_string(xml).compile()


def test_more_than_64_bodies_are_rejected():
  b = zoo.Builder(1)
  b.grow(b.body(None, (0, 0, 1), [b.joint("hinge")]), 63, max_children=8)
  with pytest.raises(ValueError, match="at most 64 bodies"):
    b.compile()


def _create_error(m) -> bytes:
  """mjx_model_create's error for a compiled model.  Its checks of the model come before it
  touches a device, so without a GPU an admitted model fails later, with a HIP error."""
  from mjlab_amd._capi import make_desc
  from mjlab_amd._lib import lib
  desc, keep = make_desc(m)
  ptr = ctypes.c_void_p()
  status = lib().mjx_model_create(ctypes.byref(desc), 0, ctypes.byref(ptr))
  del keep
  if status == 0:
    lib().mjx_model_destroy(ptr)
    return b""
  return lib().mjx_last_error()


_REFUSALS = (b"at most", b"a tree that follows", b"not supported")


@pytest.mark.parametrize("name", zoo.NAMES)
def test_engine_refuses_exactly_what_it_cannot_compute(name):
  err = _create_error(zoo.get(name).model)
  if name in zoo.REJECTED:
    assert zoo.REJECTED[name].encode() in err, err
  else:
    assert not any(w in err for w in _REFUSALS), err


def test_rejected_models_are_the_ones_with_the_defects():
  """The two conditions, restated on the compiled arrays: more than 60 dofs; a body whose root's
  level-order lane is not its id while that lane or the root holds a free body."""
  for name in zoo.NAMES:
    m = zoo.get(name).model
    lb, roots = np.asarray(m.arrays["level_body"]), np.asarray(m.body_rootid)
    free = lambda b: m.arrays["body_jntnum"][b] > 0 and m.jnt_type[m.arrays["body_jntadr"][b]] == zoo.JNT_FREE
    lane = any(lb[r] != r and (free(r) or free(lb[r])) for r in roots[1:])
    assert (name in zoo.REJECTED) == (m.nv > 60 or lane), name


def test_shipped_scenes_are_admitted():
  import glob
  from mjlab_amd.scenes import load_scene
  assets = os.path.join(ROOT, "mjlab-1_amd", "mjlab_amd", "assets", "*.npz")
  scenes = sorted(os.path.splitext(os.path.basename(f))[0] for f in glob.glob(assets))
  assert len(scenes) >= 9
  for scene in scenes:
    err = _create_error(load_scene(scene))
    assert not any(w in err for w in _REFUSALS), (scene, err)


def test_more_than_64_dofs_are_rejected():
  """Eleven free bodies: 12 bodies, 66 dofs.  mjx_model_create refuses before it touches a device."""
  from mjlab_amd._capi import make_desc
  from mjlab_amd._lib import lib
  b = zoo.Builder(2)
  for k in range(11):
    b.free_root((0.3 * k - 1.5, 0.0, 0.5))
  m = b.compile()
  assert m.nv == 66 and m.nbody == 12
  desc, keep = make_desc(m)
  ptr = ctypes.c_void_p()
  assert lib().mjx_model_create(ctypes.byref(desc), 0, ctypes.byref(ptr)) != 0
  assert b"at most 64 dofs" in lib().mjx_last_error()
  del keep
