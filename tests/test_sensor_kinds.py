"""Extended builtin sensors, the host side (no GPU): what the scene compiler makes of every
kind x object type x ref combination, from a BuiltinSensorCfg and from XML; the kinds' semantics
(tests/sensor_ref.py) pinned by algebra and calculus on the CPU oracle's fp64 fields; the cutoff;
and the descriptor checks of mjx_model_create."""

import ctypes

import numpy as np
import pytest

import oracle_lib
import sensor_probe as probe
import sensor_ref as ref
from invariants import integrate_pos
from mjlab_amd.compiler.model import REFUSED_SENSORS
from mjlab_amd.entity import EntityCfg
from mjlab_amd.scene import Scene, SceneCfg
from mjlab_amd.sensor import BuiltinSensorCfg, ObjRef
from mjlab_amd.spec import Spec

TYPES = {"gyro": 0, "velocimeter": 1, "accelerometer": 2, "framepos": 9, "framequat": 6,
         "framexaxis": 10, "frameyaxis": 11, "framezaxis": 12, "framelinvel": 13, "frameangvel": 14,
         "framelinacc": 15, "frameangacc": 16, "subtreecom": 17, "subtreelinvel": 18,
         "actuatorpos": 19, "actuatorvel": 20, "actuatorfrc": 21, "jointactuatorfrc": 22}
OBJ = {"body": 1, "xbody": 2, "joint": 3, "geom": 5, "site": 6, "actuator": 19}


def expected_arrays(m, sensors, prefix=""):
  """The sensor arrays the compiler must produce for a probe sensor list, from the rules of
  include/mjx355.h alone."""
  index = {"body": m.names["body"], "xbody": m.names["body"], "geom": m.names["geom"],
           "site": m.names["site"], "joint": m.names["joint"], "actuator": m.names["actuator"]}
  rows, adr = [], 0
  for tag, name, (ot, on), r, cutoff in sensors:
    st, otype = TYPES[tag], OBJ[ot]
    if tag == "framepos" and r is None and ot in ("site", "xbody"):
      st, otype = 5, (6 if ot == "site" else 1)  # the step kernels' framepos, as ever
    dim = 4 if tag == "framequat" else 1 if tag.startswith(("actuator", "jointactuator")) else 3
    rt, ri = (OBJ[r[0]], index[r[0]].index(prefix + r[1])) if r else (0, -1)
    rows.append((st, otype, index[ot].index(prefix + on), rt, ri, adr, dim, cutoff))
    adr += dim
  return np.array(rows, float)


def compiled_arrays(m):
  cut = np.asarray(m.arrays.get("sensor_cutoff", np.zeros(m.nsensor)), float)
  return np.stack([np.asarray(m.arrays[k], float) for k in
                   ("sensor_type", "sensor_objtype", "sensor_objid", "sensor_reftype", "sensor_refid",
                    "sensor_adr", "sensor_dim")] + [cut], axis=1)


# ------------------------------------------------------------------------------ 1. compilation
def test_every_combination_compiles_from_xml():
  sensors = probe.sensor_list()
  m = probe.probe_model(sensors)
  assert m.names["sensor"] == [s[1] for s in sensors]
  np.testing.assert_array_equal(compiled_arrays(m), expected_arrays(m, sensors))
  assert m.nsensordata == int(np.sum(m.sensor_dim))
  # extended sensors enough for more than one wave of them (tests/test_gpu_sensor_kinds.py)
  assert sum(ref.extended(t) for t in m.sensor_type) >= 70


def test_every_combination_compiles_from_cfg_with_prefixed_names():
  sensors = probe.sensor_list()
  cfgs = tuple(BuiltinSensorCfg(name=name, sensor_type=tag, obj=ObjRef(ot, on, entity="robot"),
                                ref=ObjRef(r[0], r[1], entity="robot") if r else None, cutoff=cutoff)
               for tag, name, (ot, on), r, cutoff in sensors)
  ent = EntityCfg(spec_fn=lambda: probe.probe_spec(()))
  m = Scene(SceneCfg(num_envs=1, entities={"robot": ent}, sensors=cfgs), "cpu").compile()
  assert m.names["sensor"] == ["robot/" + s[1] for s in sensors]
  np.testing.assert_array_equal(compiled_arrays(m), expected_arrays(m, sensors, "robot/"))


def test_attach_prefixes_object_and_ref_names():
  """XML sensors of an attached entity: objname, refname and actuator= follow the prefix."""
  sensors = probe.sensor_list()
  ent = EntityCfg(spec_fn=lambda: probe.probe_spec(sensors))
  m = Scene(SceneCfg(num_envs=1, entities={"robot": ent}), "cpu").compile()
  assert m.names["sensor"] == ["robot/" + s[1] for s in sensors]
  np.testing.assert_array_equal(compiled_arrays(m), expected_arrays(m, sensors, "robot/"))


def test_xml_shorthand_keeps_the_body_frame():
  """<framepos body=...> is the body's own frame, as it always was (the step kernels'
  framepos); <framequat body=...> follows it; only objtype="body" is the inertial frame."""
  xml = probe.BODY_XML.replace("__SENSORS__", """
    <framepos name="a" body="fore"/> <framequat name="b" body="fore"/>
    <framepos name="c" objtype="body" objname="fore"/> <framequat name="d" objtype="body" objname="fore"/>""")
  m = Spec.from_string(xml).compile()
  fore = m.names["body"].index("fore")
  assert m.sensor_type.tolist() == [5, 6, 9, 6]
  assert m.sensor_objtype.tolist() == [1, 2, 1, 1]
  assert m.sensor_objid.tolist() == [fore] * 4
  assert "sensor_cutoff" not in m.arrays  # a model without cutoffs keeps the arrays it had


REFUSED = sorted(REFUSED_SENSORS)


def test_the_refused_kinds_are_the_issues_list():
  assert REFUSED == sorted(["jointlimitpos", "jointlimitvel", "clock", "jointlimitfrc", "force",
                            "torque", "magnetometer", "rangefinder", "tendonpos", "tendonvel",
                            "tendonactuatorfrc", "e_potential", "e_kinetic"])


@pytest.mark.parametrize("kind", REFUSED)
def test_refused_kinds_raise_with_their_name(kind):
  site_kinds = ("force", "torque", "magnetometer", "rangefinder")
  obj = ("site", "sbase") if kind in site_kinds else ("joint", "hinge") if kind.startswith("joint") \
      else ("tendon", "t") if kind.startswith("tendon") else None
  cfg = BuiltinSensorCfg(name="x", sensor_type=kind, obj=ObjRef(*obj) if obj else None)
  with pytest.raises(NotImplementedError, match=kind):
    cfg.expand({})
  attr = f'{obj[0]}="{obj[1]}"' if obj else ""
  xml = probe.BODY_XML.replace("__SENSORS__", f'<{kind} name="x" {attr}/>')
  with pytest.raises(NotImplementedError, match=kind):
    Spec.from_string(xml).compile()


@pytest.mark.parametrize("kind", ["framelinacc", "frameangacc"])
def test_ref_on_accelerations_and_camera_frames_are_refused(kind):
  cfg = BuiltinSensorCfg(name="x", sensor_type=kind, obj=ObjRef("site", "sfore"), ref=ObjRef("xbody", "base"))
  with pytest.raises(NotImplementedError, match=kind):
    cfg.expand({})
  xml = probe.BODY_XML.replace(
    "__SENSORS__", f'<{kind} name="x" objtype="site" objname="sfore" reftype="xbody" refname="base"/>')
  with pytest.raises(NotImplementedError, match=kind):
    Spec.from_string(xml).compile()
  with pytest.raises(NotImplementedError, match="camera"):
    BuiltinSensorCfg(name="x", sensor_type=kind, obj=ObjRef("camera", "c")).expand({})
  xml = probe.BODY_XML.replace("__SENSORS__", f'<{kind} name="x" objtype="camera" objname="c"/>')
  with pytest.raises(NotImplementedError, match="camera"):
    Spec.from_string(xml).compile()


# -------------------------------------------------------------------------------- 2. semantics
NSTATE, H = 20, 1e-4


@pytest.fixture(scope="module")
def oracle_states():
  """The probe robot with the three site sensors the oracle evaluates, at NSTATE random
  states: the oracle's fp64 fields at each state and at qpos -+ H qvel."""
  sensors = [s for s in probe.sensor_list() if s[1] in ("gyro", "velocimeter", "accelerometer")]
  m = probe.probe_model(sensors)
  q, v, ctrl = probe.random_states(m, NSTATE, seed=11)
  out = []
  for i in range(NSTATE):
    mid = oracle_lib.forward(m, q[i], v[i], ctrl=ctrl[i])
    lo = oracle_lib.forward(m, integrate_pos(m, q[i], v[i], -H), v[i], ctrl=ctrl[i])
    hi = oracle_lib.forward(m, integrate_pos(m, q[i], v[i], H), v[i], ctrl=ctrl[i])
    out.append((mid, lo, hi))
  return m, out


def _value(m, d, tag, obj, r=None):
  F = ref.Frames({k: d[k] for k in ("xpos", "xquat", "cvel", "cacc", "subtree_com")}, m.arrays)
  ix = lambda t, n: (m.names["body"] if t in ("body", "xbody") else m.names[t]).index(n)
  st = TYPES[tag]
  return ref.sensor_value(F, st, OBJ[obj[0]], ix(*obj), OBJ[r[0]] if r else 0, ix(*r) if r else -1)[0]


def test_site_sensors_reappear_as_frame_sensors(oracle_states):
  """R_site gyro == frameangvel(site), R_site velocimeter == framelinvel(site), R_site
  accelerometer == framelinacc(site): algebraic identities on the oracle's sensordata."""
  m, states = oracle_states
  imu = ("site", "imu")
  for mid, _, _ in states:
    F = ref.Frames({k: mid[k] for k in ("xpos", "xquat")}, m.arrays)
    R = F.mat(ref.OBJ_SITE, m.names["site"].index("imu"))
    for k, (sens, tag) in enumerate((("gyro", "frameangvel"), ("velocimeter", "framelinvel"),
                                     ("accelerometer", "framelinacc"))):
      assert m.names["sensor"][k] == sens
      got, want = _value(m, mid, tag, imu), R @ mid["sensordata"][3 * k:3 * k + 3]
      assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (tag, got, want)


PAIRS = [(o, None) for o in probe.OBJS] + [(o, r) for o in probe.OBJS for r in probe.REFS]


@pytest.mark.parametrize("obj,r", PAIRS, ids=[f"{o[0]}-{r[0] if r else 'world'}" for o, r in PAIRS])
def test_velocities_are_the_derivatives_of_the_positions(oracle_states, obj, r):
  """framelinvel = d/dt framepos and frameangvel = 2 vec(dq/dt q^-1) of framequat, same object
  and ref, by central differences along qpos -+ H qvel.  The truncation is H^2 / 6 |d3/dt3|,
  about 2e-7 at these rates (|w| <= 5 rad/s, arms of a few 0.1 m); a wrong sign is O(1)."""
  m, states = oracle_states
  for mid, lo, hi in states:
    lin = _value(m, mid, "framelinvel", obj, r)
    fd = (_value(m, hi, "framepos", obj, r) - _value(m, lo, "framepos", obj, r)) / (2 * H)
    assert np.abs(lin - fd).max() <= 1e-5 * (1 + np.abs(lin).max()), (obj, r, lin, fd)
    ang = _value(m, mid, "frameangvel", obj, r)
    q0 = _value(m, mid, "framequat", obj, r)
    dq = (_value(m, hi, "framequat", obj, r) - _value(m, lo, "framequat", obj, r)) / (2 * H)
    # q(t) maps frame to ref coordinates, frameangvel is in ref coordinates: w = 2 dq q^-1
    w = 2 * ref.quat_mul(dq, ref.quat_conj(q0))[1:] / (q0 @ q0)
    assert np.abs(ang - w).max() <= 1e-5 * (1 + np.abs(ang).max()), (obj, r, ang, w)


def test_axes_are_the_columns_of_the_quaternions_matrix(oracle_states):
  m, states = oracle_states
  for obj, r in PAIRS:
    mid = states[0][0]
    R = ref.quat_mat(_value(m, mid, "framequat", obj, r))
    for k, tag in enumerate(("framexaxis", "frameyaxis", "framezaxis")):
      np.testing.assert_allclose(_value(m, mid, tag, obj, r), R[:, k], atol=1e-12)


# ---------------------------------------------------------------------------------- 3. cutoff
def test_cutoff_clamps_real_kinds_and_spares_quaternions_and_axes(oracle_states):
  _, states = oracle_states
  sensors = [s for s in probe.sensor_list() if s[4] > 0 and s[0] != "gyro"]
  plain = [(t, n, o, r, 0.0) for t, n, o, r, _ in sensors]
  mc, mp = probe.probe_model(sensors), probe.probe_model(plain)
  assert mc.arrays["sensor_cutoff"].tolist() == [s[4] for s in sensors]
  assert "sensor_cutoff" not in mp.arrays
  clamped = 0
  for mid, _, _ in states:
    d = dict(mid, subtree_linvel=np.zeros((mc.nbody, 3)), actuator_length=np.zeros(mc.nu),
             actuator_velocity=np.zeros(mc.nu), qfrc_actuator=np.zeros(mc.nv))
    d.pop("sensordata")
    vc = ref.evaluate(mc.arrays, d)[0]
    vp = ref.evaluate(mp.arrays, d)[0]
    for s, (tag, name, _, _, cutoff) in enumerate(sensors):
      a, k = int(mc.sensor_adr[s]), int(mc.sensor_dim[s])
      if tag in ("framequat", "framezaxis"):
        np.testing.assert_array_equal(vc[a:a + k], vp[a:a + k])
      else:
        np.testing.assert_array_equal(vc[a:a + k], np.clip(vp[a:a + k], -cutoff, cutoff))
        clamped += int((np.abs(vp[a:a + k]) > cutoff).sum())
  assert clamped > 0  # the cutoffs bite at these states


# ------------------------------------------------------------------ descriptor checks (C ABI)
def _create(model):
  from mjlab_amd._capi import make_desc
  from mjlab_amd._lib import lib
  L = lib()
  desc, keep = make_desc(model)
  out = ctypes.c_void_p()
  status = L.mjx_model_create(ctypes.byref(desc), 0, ctypes.byref(out))
  del keep
  return status, L.mjx_last_error().decode(), out


@pytest.mark.parametrize("field,value,word", [("sensor_objid", 1000, "object"), ("sensor_objid", -1, "object"),
                                              ("sensor_refid", 1000, "ref"), ("sensor_refid", -2, "ref")])
def test_model_create_rejects_ids_out_of_range(field, value, word):
  """A bad object or ref id is an error code from mjx_model_create, before any device work."""
  sensors = [("framelinvel", "x", ("geom", "garm"), ("site", "sbase"), 0.0)]
  m = probe.probe_model(sensors)
  m.arrays[field] = np.array([value], np.int32)
  status, err, _ = _create(m)
  assert status != 0 and word in err, err
