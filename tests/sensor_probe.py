"""The probe robot of the extended-sensor tests (tests/test_sensor_kinds.py, tests/
test_gpu_sensor_kinds.py): a free box base, a hinge arm, a slide forearm (a grandchild with an
off-centre, rotated <inertial>), a second hinge leg; sites and geoms with rotated local frames;
three position actuators with gear != 1; and a sensor list that covers every extended kind on
every object type, every (object type, ref type) pair, the non-frame kinds, and cutoffs."""

import numpy as np

BODY_XML = """
<mujoco model="probe">
  <worldbody>
    <body name="base" pos="0 0 0.5" quat="0.98 0.1 -0.12 0.08">
      <freejoint name="root"/>
      <geom name="gbase" type="box" size="0.15 0.1 0.05" pos="0.01 0.02 0" quat="0.95 0.1 0.2 0.15" mass="3"/>
      <site name="sbase" pos="0.05 -0.03 0.04" quat="0.9 0.3 0.1 0.2"/>
      <body name="arm" pos="0.2 0 0.05" quat="0.98 0 0.2 0">
        <joint name="hinge" type="hinge" axis="0 1 0" pos="0 0 0.01" damping="0.2"/>
        <geom name="garm" type="capsule" size="0.03 0.1" pos="0.1 0 0" quat="0.7 0 0.7 0.1" mass="1"/>
        <site name="sarm" pos="0.08 0.01 0.02" quat="0.8 -0.2 0.5 0.1"/>
        <body name="fore" pos="0.22 0 0" quat="0.96 0.2 0 0.1">
          <joint name="slide" type="slide" axis="1 0 0.2" damping="1"/>
          <inertial pos="0.03 -0.02 0.01" quat="0.85 0.3 -0.2 0.35" mass="0.6" diaginertia="0.002 0.003 0.0015"/>
          <geom name="gfore" type="sphere" size="0.04" pos="0.02 0 0.01" quat="0.6 0.5 -0.4 0.3"/>
          <site name="sfore" pos="0.03 0.02 -0.01" quat="0.5 0.5 -0.6 0.3"/>
          <site name="imu" pos="-0.02 0.01 0.03" quat="0.7 -0.1 0.3 0.6"/>
        </body>
      </body>
      <body name="leg" pos="-0.1 0.05 -0.05" quat="0.9 0.3 0 -0.2">
        <joint name="knee" type="hinge" axis="1 0.2 0" damping="0.2"/>
        <geom name="gleg" type="capsule" size="0.025 0.08" pos="0 0 -0.1" quat="0.99 0.1 0 0" mass="0.8"/>
      </body>
    </body>
  </worldbody>
  <sensor>
__SENSORS__
  </sensor>
</mujoco>
"""

FRAME_KINDS = ("framepos", "framequat", "framexaxis", "frameyaxis", "framezaxis", "framelinvel",
               "frameangvel", "framelinacc", "frameangacc")
REF_KINDS = FRAME_KINDS[:7]
OBJS = (("xbody", "fore"), ("body", "fore"), ("geom", "garm"), ("site", "sfore"))
REFS = (("xbody", "base"), ("body", "arm"), ("geom", "gbase"), ("site", "sbase"))
ACTUATORS = (("hinge", 3.0), ("slide", 0.5), ("knee", -2.0))  # joint, gear


def sensor_list():
  """[(tag, name, obj (type, name), ref (type, name) | None, cutoff)] of the probe robot."""
  out = []
  for k in FRAME_KINDS:
    for t, n in OBJS:
      out.append((k, f"{k}_{t}", (t, n), None, 0.0))
  for i, k in enumerate(REF_KINDS):  # kind i pairs object type o with ref type (o + i) % 4:
    for o, (t, n) in enumerate(OBJS):  # the first four kinds cover all sixteen pairs
      rt, rn = REFS[(o + i) % 4]
      out.append((k, f"{k}_{t}_in_{rt}", (t, n), (rt, rn), 0.0))
  for k in ("subtreecom", "subtreelinvel"):
    for b in ("base", "arm"):
      out.append((k, f"{k}_{b}", ("body", b), None, 0.0))
  for k in ("actuatorpos", "actuatorvel", "actuatorfrc"):
    for j, _ in ACTUATORS:
      out.append((k, f"{k}_{j}", ("actuator", j), None, 0.0))
  for j in ("hinge", "slide"):
    out.append(("jointactuatorfrc", f"jointactuatorfrc_{j}", ("joint", j), None, 0.0))
  # the step kernels' sensors at one shared site (identities), a cutoff on one of them, cutoffs
  # on new kinds, and cutoffs a quaternion and an axis must ignore
  for k in ("gyro", "velocimeter", "accelerometer"):
    out.append((k, k, ("site", "imu"), None, 0.0))
  for k in ("frameangvel", "framelinvel", "framelinacc", "framepos"):
    out.append((k, f"{k}_imu", ("site", "imu"), None, 0.0))
  out.append(("gyro", "gyro_cut", ("site", "imu"), None, 0.3))
  out.append(("framelinvel", "linvel_cut", ("geom", "garm"), None, 0.05))
  out.append(("framepos", "pos_cut", ("body", "fore"), ("site", "sbase"), 0.1))
  out.append(("actuatorfrc", "frc_cut", ("actuator", "hinge"), None, 0.2))
  out.append(("framequat", "quat_cut", ("body", "fore"), None, 0.1))
  out.append(("framezaxis", "zaxis_cut", ("site", "sfore"), None, 0.1))
  return out


def sensor_xml(sensors):
  lines = []
  for tag, name, (ot, on), ref, cutoff in sensors:
    if ot in ("site", "joint", "actuator") and tag not in FRAME_KINDS or tag.startswith("subtree"):
      a = f'{ot}="{on}"'
    else:
      a = f'objtype="{ot}" objname="{on}"'
    if ref is not None:
      a += f' reftype="{ref[0]}" refname="{ref[1]}"'
    if cutoff > 0:
      a += f' cutoff="{cutoff}"'
    lines.append(f'    <{tag} name="{name}" {a}/>')
  return "\n".join(lines)


def probe_spec(sensors=None):
  """The probe robot as a Spec: its sensors in the XML (`sensors`: a sensor_list(), None: all
  of it, (): none), its actuators added through the spec API."""
  from mjlab_amd.spec import Spec, create_position_actuator
  sensors = sensor_list() if sensors is None else sensors
  spec = Spec.from_string(BODY_XML.replace("__SENSORS__", sensor_xml(sensors)))
  for j, gear in ACTUATORS:
    create_position_actuator(spec, j, stiffness=20.0, damping=1.0).gear[0] = gear
  return spec


def probe_model(sensors=None):
  m = probe_spec(sensors).compile(terrain="plane")
  return m


def random_states(m, n, seed, wmax=5.0):
  """n random states: the base above the plane with a random attitude, joints in a moderate
  range, |angular velocities| <= wmax rad/s."""
  rng = np.random.default_rng(seed)
  q = np.tile(np.asarray(m.qpos0, float), (n, 1))
  q[:, 2] = 0.55 + 0.1 * rng.random(n)
  quat = rng.normal(size=(n, 4))
  q[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
  q[:, 7:] = rng.uniform(-0.4, 0.4, (n, m.nq - 7)) * np.array([1.0, 0.2, 1.0])
  v = np.zeros((n, m.nv))
  v[:, :3] = rng.uniform(-1, 1, (n, 3))
  w = rng.normal(size=(n, 3))
  v[:, 3:6] = w / np.linalg.norm(w, axis=1, keepdims=True) * rng.uniform(0, wmax, (n, 1))
  v[:, 6:] = rng.uniform(-2, 2, (n, m.nv - 6)) * np.array([1.0, 0.3, 1.0])
  ctrl = rng.uniform(-0.5, 0.5, (n, m.nu))
  return q, v, ctrl


def sensor_kinds_g1_cfg(num_envs: int = 64):
  """The shipped G1 velocity task with six extended sensors added through cfg.scene.sensors
  (tests/test_gpu_sensor_kinds.py; __graft_entry__.build() compiles the run-time specialised
  kernels of this scene, whose sensor counts match no compiled specs.inc entry)."""
  from mjlab_amd.envs import load_env_cfg
  from mjlab_amd.sensor import BuiltinSensorCfg, ObjRef
  cfg = load_env_cfg("Mjlab-Velocity-Flat-Unitree-G1")
  cfg.scene.num_envs = num_envs
  o = lambda t, n: ObjRef(t, n, entity="robot")
  cfg.scene.sensors = cfg.scene.sensors + (
    BuiltinSensorCfg("x_com", "subtreecom", o("body", "pelvis")),
    BuiltinSensorCfg("x_foot_in_pelvis", "framepos", o("site", "left_foot"), ref=o("xbody", "pelvis")),
    BuiltinSensorCfg("x_torso_quat", "framequat", o("xbody", "torso_link")),
    BuiltinSensorCfg("x_foot_vel", "framelinvel", o("site", "right_foot"), ref=o("site", "imu_in_pelvis")),
    BuiltinSensorCfg("x_palm_acc", "framelinacc", o("site", "left_palm"), cutoff=50.0),
    BuiltinSensorCfg("x_knee_frc", "jointactuatorfrc", o("joint", "left_knee_joint")))
  return cfg
