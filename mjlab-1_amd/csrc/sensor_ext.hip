// sensor_ext.hip — the extended sensors (include/mjx355.h MJX_SENS_FRAMEPOSX and later, every
// MJX_SENS_FRAMEQUAT, ref frames, cutoffs): one small kernel behind the step's last launch.
//
// Its inputs are fields the last substep (or a forward) has stored in HBM -- the body, inertial,
// geom and site frames, cvel, cacc, subtree_com, subtree_linvel, actuator_* and qfrc_actuator --
// so no step kernel changes for it; it writes sensordata only.
//
// Thread mapping: a lane is a world, blockIdx.y an extended sensor.  The sensor's record, and
// with it the kind, the object types and every branch below, is uniform over the wave (scalar
// loads, no divergence); the lanes of a wave read the same field entry of 64 consecutive
// worlds.  Those reads are strided by a world's field size, which a kernel of a few loads per
// lane can afford; the other mapping (a lane per sensor, a workgroup per world) would leave
// most of a wave idle at the usual handful of sensors and diverge over their kinds.
#include "engine.h"

#include <atomic>

namespace mjx {
namespace {

struct V3 { float x, y, z; };
struct Q4 { float w, x, y, z; };
__device__ inline V3 ld3(const float* p) { return {p[0], p[1], p[2]}; }
__device__ inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline V3 cross(V3 a, V3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// R^T v, R row-major
__device__ inline V3 mulTv(const float* R, V3 v) {
  return {R[0] * v.x + R[3] * v.y + R[6] * v.z, R[1] * v.x + R[4] * v.y + R[7] * v.z,
          R[2] * v.x + R[5] * v.y + R[8] * v.z};
}
__device__ inline Q4 qmul(Q4 a, Q4 b) {
  return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}

// A frame of world w: position, rotation matrix and quaternion by object type (BODY: the
// inertial frame), and the point kinematics of a frame's origin, in world orientation.
struct Frames {
  const Params& P;
  size_t w;
  __device__ const float* pos(int type, int id) const {
    const Dims& d = P.d;
    return type == OBJ_XBODY  ? P.D.xpos + (w * d.nbody + id) * 3
           : type == OBJ_BODY ? P.D.xipos + (w * d.nbody + id) * 3
           : type == OBJ_GEOM ? P.D.geom_xpos + (w * d.ngeom + id) * 3
                              : P.D.site_xpos + (w * d.nsite + id) * 3;
  }
  __device__ const float* mat(int type, int id) const {
    const Dims& d = P.d;
    return type == OBJ_XBODY  ? P.D.xmat + (w * d.nbody + id) * 9
           : type == OBJ_BODY ? P.D.ximat + (w * d.nbody + id) * 9
           : type == OBJ_GEOM ? P.D.geom_xmat + (w * d.ngeom + id) * 9
                              : P.D.site_xmat + (w * d.nsite + id) * 9;
  }
  __device__ Q4 quat(int type, int id, int body) const {
    const float* xq = P.D.xquat + (w * P.d.nbody + body) * 4;
    const Q4 qb = {xq[0], xq[1], xq[2], xq[3]};
    if (type == OBJ_XBODY) return qb;
    const DModel& m = P.m;
    const float* l = type == OBJ_BODY   ? m.body_iquat + w * m.body_iquat_ws + 4 * id
                     : type == OBJ_GEOM ? m.geom_quat + w * m.geom_quat_ws + 4 * id
                                        : m.site_quat + w * m.site_quat_ws + 4 * id;
    return qmul(qb, Q4{l[0], l[1], l[2], l[3]});
  }
  __device__ V3 angvel(int body) const { return ld3(P.D.cvel + (w * P.d.nbody + body) * 6); }
  __device__ V3 angacc(int body) const { return ld3(P.D.cacc + (w * P.d.nbody + body) * 6); }
  // p - subtree_com[root]: the arm of the body's spatial velocity / acceleration
  __device__ V3 arm(V3 p, int root) const { return p - ld3(P.D.subtree_com + (w * P.d.nbody + root) * 3); }
  __device__ V3 linvel(int body, V3 rel) const {
    const float* cv = P.D.cvel + (w * P.d.nbody + body) * 6;
    return ld3(cv + 3) + cross(ld3(cv), rel);
  }
  __device__ V3 linacc(int body, V3 rel) const {
    const float* ca = P.D.cacc + (w * P.d.nbody + body) * 6;
    return ld3(ca + 3) + cross(ld3(ca), rel) + cross(angvel(body), linvel(body, rel));
  }
};

__device__ inline float clampc(float v, float c) { return c > 0.f ? fminf(fmaxf(v, -c), c) : v; }

}  // namespace

__global__ __launch_bounds__(kWave) void sensor_ext_kernel(const Params* __restrict__ Pp,
                                                           const SensorExtRec* __restrict__ rec,
                                                           int nworld, const uint8_t* __restrict__ mask) {
  const int wi = blockIdx.x * kWave + threadIdx.x;
  if (wi >= nworld) return;
  if (mask && !mask[wi]) return;
  const Params& P = *Pp;
  const SensorExtRec r = rec[blockIdx.y];
  const Dims& d = P.d;
  const size_t w = (size_t)wi;
  const Frames F{P, w};
  float* out = P.D.sensordata + w * d.nsensordata + r.adr;
  const bool ref = r.rtype != OBJ_NONE;
  const float c = r.cutoff;
  V3 v;
  switch (r.kind) {
    case kSensClamp:  // a kind the step kernels wrote: its cutoff
      for (int i = 0; i < r.dim; i++) out[i] = clampc(out[i], c);
      return;
    case SENS_FRAMEQUAT: {
      Q4 q = F.quat(r.otype, r.oid, r.obody);
      if (ref) {
        const Q4 qr = F.quat(r.rtype, r.rid, r.rbody);
        q = qmul(Q4{qr.w, -qr.x, -qr.y, -qr.z}, q);
      }
      out[0] = q.w; out[1] = q.x; out[2] = q.y; out[3] = q.z;
      return;
    }
    case SENS_FRAMEPOSX:
      v = ld3(F.pos(r.otype, r.oid));
      if (ref) v = mulTv(F.mat(r.rtype, r.rid), v - ld3(F.pos(r.rtype, r.rid)));
      break;
    case SENS_FRAMEXAXIS:
    case SENS_FRAMEYAXIS:
    case SENS_FRAMEZAXIS: {
      const float* R = F.mat(r.otype, r.oid) + (r.kind - SENS_FRAMEXAXIS);
      v = V3{R[0], R[3], R[6]};
      if (ref) v = mulTv(F.mat(r.rtype, r.rid), v);
      break;
    }
    case SENS_FRAMELINVEL: {
      const V3 po = ld3(F.pos(r.otype, r.oid));
      v = F.linvel(r.obody, F.arm(po, r.oroot));
      if (ref) {
        const V3 pr = ld3(F.pos(r.rtype, r.rid));
        const V3 vr = F.linvel(r.rbody, F.arm(pr, r.rroot));
        v = mulTv(F.mat(r.rtype, r.rid), v - vr - cross(F.angvel(r.rbody), po - pr));
      }
      break;
    }
    case SENS_FRAMEANGVEL:
      v = F.angvel(r.obody);
      if (ref) v = mulTv(F.mat(r.rtype, r.rid), v - F.angvel(r.rbody));
      break;
    case SENS_FRAMELINACC:
      v = F.linacc(r.obody, F.arm(ld3(F.pos(r.otype, r.oid)), r.oroot));
      break;
    case SENS_FRAMEANGACC:
      v = F.angacc(r.obody);
      break;
    case SENS_SUBTREECOM:
      v = ld3(P.D.subtree_com + (w * d.nbody + r.oid) * 3);
      break;
    case SENS_SUBTREELINVEL:
      v = ld3(P.D.subtree_linvel + (w * d.nbody + r.oid) * 3);
      break;
    case SENS_ACTUATORPOS:
      out[0] = clampc(P.D.actuator_length[w * d.nu + r.oid], c);
      return;
    case SENS_ACTUATORVEL:
      out[0] = clampc(P.D.actuator_velocity[w * d.nu + r.oid], c);
      return;
    case SENS_ACTUATORFRC:
      out[0] = clampc(P.D.actuator_force[w * d.nu + r.oid], c);
      return;
    case SENS_JOINTACTUATORFRC:  // oid: the joint's dof (capi.cpp)
      out[0] = clampc(P.D.qfrc_actuator[w * d.nv + r.oid], c);
      return;
    default:
      return;  // (mjx_model_create lists no other kind)
  }
  out[0] = clampc(v.x, c); out[1] = clampc(v.y, c); out[2] = clampc(v.z, c);
}

// Launches issued by this process (host side; mjx_sensor_launch_count), apart from the step
// kernels' counters, whose layout is fixed.
static std::atomic<long long> g_sensor_ext_launches{0};
long long sensor_ext_launches() { return g_sensor_ext_launches.load(std::memory_order_relaxed); }
void sensor_ext_launches_reset() { g_sensor_ext_launches.store(0, std::memory_order_relaxed); }

hipError_t launch_sensor_ext(const Params* dev, const SensorExt& ext, int nworld,
                             const uint8_t* mask, hipStream_t stream) {
  if (ext.n <= 0 || nworld <= 0) return hipSuccess;
  g_sensor_ext_launches.fetch_add(1, std::memory_order_relaxed);
  hipLaunchKernelGGL(sensor_ext_kernel, dim3((nworld + kWave - 1) / kWave, ext.n), dim3(kWave), 0,
                     stream, dev, ext.rec, nworld, mask);
  return hipGetLastError();
}

}  // namespace mjx
