"""fp64 reference of the extended sensors (include/mjx355.h MJX_SENS_FRAMEPOSX and later, every
MJX_SENS_FRAMEQUAT, ref frames, cutoffs), from the data fields (one world's, or a batch with
leading world axes) and the model arrays.

`evaluate` returns, per sensordata entry, the value and a magnitude T: the value of the same
formula with every input replaced by its absolute value and every subtraction by an addition,
i.e. the sum of the absolute values of the terms the formula adds.  A kernel that evaluates the
formula in fp32 with at most n roundings on any path from an input to the entry is within
n * 2^-24 * T of the fp64 value of the same (fp32) inputs (each rounding is relative to an
intermediate no larger than its own T, and the later operations scale it by at most their
absolute factors, which T already carries).

ROUNDINGS: n per kind, (without ref, with ref), counted on csrc/sensor_ext.hip:
  cross(a, b): one product and one subtraction per entry            -> depth(a, b) + 2
  R^T v: a product and two additions per entry                      -> depth(v) + 3
  q1 * q2: a product and three additions / subtractions per entry   -> depth(q) + 4
  p - c (the arm of cvel / cacc)                                    -> 1
  v = lin + w x (p - c)                                             -> 1 + 2 + 1 = 4
  a = (lin' + w' x (p - c)) + w x v: w x v is at 4 + 2, the sum at  -> 7
  framepos, ref:    R_r^T (p_o - p_r)                               -> 1 + 3 = 4
  framequat:        xquat * local quat -> 4; ref: conj(q_r) * q_o   -> 4 + 4 = 8
  axes, ref:        R_r^T column                                    -> 3
  framelinvel, ref: R_r^T ((v_o - v_r) - w_r x (p_o - p_r)): 4 + 1, then max(5, 1 + 2) + 1,
                    then R^T                                        -> 6 + 3 = 9
  frameangvel, ref: R_r^T (w_o - w_r)                               -> 1 + 3 = 4
Fused multiply-adds only remove roundings; the tests allow one more (n + 1) for them.  A kind
with n = 0 is a copy and is compared bit for bit.
"""

import numpy as np

(GYRO, VELOCIMETER, ACCELEROMETER, SUBTREEANGMOM, CONTACT, FRAMEPOS, FRAMEQUAT, JOINTPOS, JOINTVEL,
 FRAMEPOSX, FRAMEXAXIS, FRAMEYAXIS, FRAMEZAXIS, FRAMELINVEL, FRAMEANGVEL, FRAMELINACC, FRAMEANGACC,
 SUBTREECOM, SUBTREELINVEL, ACTUATORPOS, ACTUATORVEL, ACTUATORFRC, JOINTACTUATORFRC) = range(23)
OBJ_NONE, OBJ_BODY, OBJ_XBODY, OBJ_JOINT, OBJ_GEOM, OBJ_SITE, OBJ_ACTUATOR = 0, 1, 2, 3, 5, 6, 19
KIND_NAMES = {FRAMEPOSX: "framepos", FRAMEQUAT: "framequat", FRAMEXAXIS: "framexaxis",
              FRAMEYAXIS: "frameyaxis", FRAMEZAXIS: "framezaxis", FRAMELINVEL: "framelinvel",
              FRAMEANGVEL: "frameangvel", FRAMELINACC: "framelinacc", FRAMEANGACC: "frameangacc",
              SUBTREECOM: "subtreecom", SUBTREELINVEL: "subtreelinvel", ACTUATORPOS: "actuatorpos",
              ACTUATORVEL: "actuatorvel", ACTUATORFRC: "actuatorfrc",
              JOINTACTUATORFRC: "jointactuatorfrc"}
ROUNDINGS = {"framepos": (0, 4), "framequat": (4, 8), "framexaxis": (0, 3), "frameyaxis": (0, 3),
             "framezaxis": (0, 3), "framelinvel": (4, 9), "frameangvel": (0, 4),
             "framelinacc": (7, None), "frameangacc": (0, None), "subtreecom": (0, None),
             "subtreelinvel": (0, None), "actuatorpos": (0, None), "actuatorvel": (0, None),
             "actuatorfrc": (0, None), "jointactuatorfrc": (0, None)}
NO_CUTOFF = (FRAMEQUAT, FRAMEXAXIS, FRAMEYAXIS, FRAMEZAXIS, CONTACT)
EPS32 = 2.0 ** -24


def extended(stype):
  """Whether the sensor kernel (not a step kernel) writes a sensor of this type."""
  return stype == FRAMEQUAT or stype >= FRAMEPOSX


# ------------------------------------------------------------------------------ small algebra
# Every array may carry leading batch (world) axes; the last axis (or two) is the object's own.
def quat_mul(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  a0, a1, a2, a3 = (a[..., i] for i in range(4))
  b0, b1, b2, b3 = (b[..., i] for i in range(4))
  return np.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                   a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1, a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], axis=-1)


def quat_conj(q):
  return np.asarray(q, np.float64) * np.array([1.0, -1.0, -1.0, -1.0])


def quat_mat(q):
  q = np.asarray(q, np.float64)
  w, x, y, z = (q[..., i] for i in range(4))
  rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
          2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
          2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
  return np.stack(rows, axis=-1).reshape(q.shape[:-1] + (3, 3))


def rot(R, v):
  """R v for R [..., 3, 3]."""
  return np.einsum("...ij,...j->...i", R, v)


# (value, magnitude) pairs
def _leaf(x):
  x = np.asarray(x, np.float64)
  return x, np.abs(x)


def _add(a, b):
  return a[0] + b[0], a[1] + b[1]


def _sub(a, b):
  return a[0] - b[0], a[1] + b[1]


def _cross(a, b):
  (x, tx), (y, ty) = a, b
  t = np.stack([tx[..., 1] * ty[..., 2] + tx[..., 2] * ty[..., 1],
                tx[..., 2] * ty[..., 0] + tx[..., 0] * ty[..., 2],
                tx[..., 0] * ty[..., 1] + tx[..., 1] * ty[..., 0]], axis=-1)
  return np.cross(x, y), t


def _rtv(R, v):
  R = np.asarray(R, np.float64)
  return np.einsum("...ji,...j->...i", R, v[0]), np.einsum("...ji,...j->...i", np.abs(R), v[1])


def _qmul(a, b):
  (x, tx), (y, ty) = a, b
  return quat_mul(x, y), _qmag(tx, ty)


def _qmag(a, b):
  """The quaternion product with every sign +."""
  a0, a1, a2, a3 = (a[..., i] for i in range(4))
  b0, b1, b2, b3 = (b[..., i] for i in range(4))
  return np.stack([a0 * b0 + a1 * b1 + a2 * b2 + a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 + a3 * b2,
                   a0 * b2 + a1 * b3 + a2 * b0 + a3 * b1, a0 * b3 + a1 * b2 + a2 * b1 + a3 * b0], axis=-1)


# ------------------------------------------------------------------------------------- frames
_WIDTH = {"xpos": 3, "xquat": 4, "xmat": 9, "xipos": 3, "ximat": 9, "geom_xpos": 3, "geom_xmat": 9,
          "site_xpos": 3, "site_xmat": 9, "cvel": 6, "cacc": 6, "subtree_com": 3, "subtree_linvel": 3}


def with_frames(d, A):
  """`d` with the inertial, geom and site frames; those it lacks are derived in fp64 from
  xpos / xquat and the model's offsets.  Fields are [..., count, width]."""
  f = {}
  for k, v in d.items():
    v = np.asarray(v, np.float64)
    if k in _WIDTH and v.shape[-1] != _WIDTH[k]:
      v = v.reshape(v.shape[:-1] + (-1, _WIDTH[k]))
    f[k] = v
  mod = lambda k, w: np.asarray(A[k], np.float64).reshape(np.asarray(A[k]).shape[:-2] + (-1, w)) \
      if np.asarray(A[k]).ndim >= 2 else np.asarray(A[k], np.float64).reshape(-1, w)
  if "xmat" not in f:
    f["xmat"] = quat_mat(f["xquat"]).reshape(f["xquat"].shape[:-1] + (9,))
  R = f["xmat"].reshape(f["xmat"].shape[:-1] + (3, 3))
  if "xipos" not in f:
    f["xipos"] = f["xpos"] + rot(R, mod("body_ipos", 3))
  if "ximat" not in f:
    q = quat_mul(f["xquat"], mod("body_iquat", 4))
    f["ximat"] = quat_mat(q).reshape(q.shape[:-1] + (9,))
  for kind in ("geom", "site"):
    bid = np.asarray(A[kind + "_bodyid"], int)
    if kind + "_xpos" not in f:
      f[kind + "_xpos"] = f["xpos"][..., bid, :] + rot(R[..., bid, :, :], mod(kind + "_pos", 3))
    if kind + "_xmat" not in f:
      q = quat_mul(f["xquat"][..., bid, :], mod(kind + "_quat", 4))
      f[kind + "_xmat"] = quat_mat(q).reshape(q.shape[:-1] + (9,))
  return f


class Frames:
  def __init__(self, d, A):
    self.f, self.A = with_frames(d, A), A

  def body(self, t, i):
    return int(self.A["geom_bodyid"][i]) if t == OBJ_GEOM else int(self.A["site_bodyid"][i]) if t == OBJ_SITE else int(i)

  def pos(self, t, i):
    return _leaf(self.f[{OBJ_XBODY: "xpos", OBJ_BODY: "xipos", OBJ_GEOM: "geom_xpos", OBJ_SITE: "site_xpos"}[t]][..., i, :])

  def mat(self, t, i):
    m = self.f[{OBJ_XBODY: "xmat", OBJ_BODY: "ximat", OBJ_GEOM: "geom_xmat", OBJ_SITE: "site_xmat"}[t]][..., i, :]
    return m.reshape(m.shape[:-1] + (3, 3))

  def quat(self, t, i):
    qb = _leaf(self.f["xquat"][..., self.body(t, i), :])
    if t == OBJ_XBODY:
      return qb
    loc = np.asarray(self.A[{OBJ_BODY: "body_iquat", OBJ_GEOM: "geom_quat", OBJ_SITE: "site_quat"}[t]], np.float64)
    return _qmul(qb, _leaf(loc[..., i, :]))

  def angvel(self, b):
    return _leaf(self.f["cvel"][..., b, :3])

  def angacc(self, b):
    return _leaf(self.f["cacc"][..., b, :3])

  def arm(self, p, b):
    return _sub(p, _leaf(self.f["subtree_com"][..., int(self.A["body_rootid"][b]), :]))

  def linvel(self, b, rel):
    return _add(_leaf(self.f["cvel"][..., b, 3:]), _cross(self.angvel(b), rel))

  def linacc(self, b, rel):
    return _add(_add(_leaf(self.f["cacc"][..., b, 3:]), _cross(self.angacc(b), rel)),
                _cross(self.angvel(b), self.linvel(b, rel)))


def sensor_value(F, stype, ot, oi, rt=OBJ_NONE, ri=-1):
  """(value, T) of one extended sensor, unclamped; [..., dim]."""
  A, f = F.A, F.f
  ref = rt != OBJ_NONE
  if stype == FRAMEQUAT:
    q = F.quat(ot, oi)
    if ref:
      qr = F.quat(rt, ri)
      q = _qmul((quat_conj(qr[0]), qr[1]), q)
    return q
  if stype == FRAMEPOSX:
    v = F.pos(ot, oi)
    return _rtv(F.mat(rt, ri), _sub(v, F.pos(rt, ri))) if ref else v
  if stype in (FRAMEXAXIS, FRAMEYAXIS, FRAMEZAXIS):
    v = _leaf(F.mat(ot, oi)[..., :, stype - FRAMEXAXIS])
    return _rtv(F.mat(rt, ri), v) if ref else v
  if stype == FRAMELINVEL:
    po, bo = F.pos(ot, oi), F.body(ot, oi)
    v = F.linvel(bo, F.arm(po, bo))
    if ref:
      pr, br = F.pos(rt, ri), F.body(rt, ri)
      vr = F.linvel(br, F.arm(pr, br))
      v = _rtv(F.mat(rt, ri), _sub(_sub(v, vr), _cross(F.angvel(br), _sub(po, pr))))
    return v
  if stype == FRAMEANGVEL:
    v = F.angvel(F.body(ot, oi))
    return _rtv(F.mat(rt, ri), _sub(v, F.angvel(F.body(rt, ri)))) if ref else v
  if stype == FRAMELINACC:
    bo = F.body(ot, oi)
    return F.linacc(bo, F.arm(F.pos(ot, oi), bo))
  if stype == FRAMEANGACC:
    return F.angacc(F.body(ot, oi))
  if stype == SUBTREECOM:
    return _leaf(f["subtree_com"][..., oi, :])
  if stype == SUBTREELINVEL:
    return _leaf(f["subtree_linvel"][..., oi, :])
  if stype in (ACTUATORPOS, ACTUATORVEL, ACTUATORFRC):
    k = {ACTUATORPOS: "actuator_length", ACTUATORVEL: "actuator_velocity", ACTUATORFRC: "actuator_force"}[stype]
    return _leaf(np.asarray(f[k])[..., oi:oi + 1])
  if stype == JOINTACTUATORFRC:
    a = int(A["jnt_dofadr"][oi])
    return _leaf(np.asarray(f["qfrc_actuator"])[..., a:a + 1])
  raise ValueError(f"sensor type {stype} is not an extended sensor")


def clamp(stype, value, cutoff):
  if cutoff > 0 and stype not in NO_CUTOFF:
    return np.clip(value, -cutoff, cutoff)
  return value


def evaluate(A, d):
  """The extended sensors: (value, T, n, written).  value and T are [..., nsensordata] over the
  data fields' leading (world) axes; n [nsensordata]: each entry's rounding count; written
  [nsensordata]: the entries an extended sensor owns.  `A`: the model arrays (sensor_*,
  body_rootid, *_bodyid, jnt_dofadr, and the local frames, shared or with the same leading
  axes as the data), `d`: the data fields."""
  F = Frames(d, A)
  nsd = int(np.sum(A["sensor_dim"]))
  lead = F.f["xpos"].shape[:-2]
  val, T = np.zeros(lead + (nsd,)), np.zeros(lead + (nsd,))
  n, own = np.zeros(nsd, int), np.zeros(nsd, bool)
  cut = np.asarray(A.get("sensor_cutoff", np.zeros(len(A["sensor_type"]))), float)
  for s, st in enumerate(np.asarray(A["sensor_type"], int)):
    if not extended(st):
      continue
    rt = int(A["sensor_reftype"][s])
    v, t = sensor_value(F, st, int(A["sensor_objtype"][s]), int(A["sensor_objid"][s]), rt,
                        int(A["sensor_refid"][s]))
    a, k = int(A["sensor_adr"][s]), int(A["sensor_dim"][s])
    val[..., a:a + k], T[..., a:a + k] = clamp(st, v, cut[s]), t
    n[a:a + k] = ROUNDINGS[KIND_NAMES[st]][1 if rt != OBJ_NONE else 0]
    own[a:a + k] = True
  return val, T, n, own
