/* mjx355 — MI355X-native batched MuJoCo step: the C ABI of the drop-in boundary.
 *
 * This header is the seam that replaces the reference's physics boundary
 * `mjlab.sim.Simulation` (src/mjlab/sim/sim.py:100-286) and the MuJoCo-Warp calls
 * behind it:
 *
 *   mjx_model_create   <- mujoco_warp.put_model(mj_model)            sim/sim.py:139
 *   mjx_sim_create     <- mujoco_warp.put_data(..., nworld, nconmax,  sim/sim.py:143-149
 *                         njmax) + create_graph()                     sim/sim.py:164-191
 *   mjx_step           <- mujoco_warp.step / wp.capture_launch        sim/sim.py:267-273
 *   mjx_forward        <- mujoco_warp.forward                         sim/sim.py:260-265
 *   mjx_reset          <- mujoco_warp.reset_data(reset=mask)          sim/sim.py:275-286
 *   mjx_field          <- WarpBridge.__getattr__ -> wp.to_torch       sim/sim_data.py:177-240
 *                         (here: a DLPack DLManagedTensor aliasing device memory)
 *   mjx_expand_field   <- expand_model_fields / repeat_array_kernel   sim/sim.py:226-240,
 *                                                                     sim/randomization.py:9-54
 *
 * Conventions: plain C, no exceptions cross the ABI, every call returns an int status
 * (0 = ok) and `mjx_last_error()` gives the message of the last failure on this thread.
 * All device work is enqueued on the HIP stream passed in (`void*` = hipStream_t, NULL =
 * legacy default stream); nothing in step/forward/reset synchronises the host.
 */
#ifndef MJX355_H_
#define MJX355_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MJX_ABI_VERSION 4

/* geom types (MuJoCo mjtGeom numbering) */
enum { MJX_GEOM_PLANE = 0, MJX_GEOM_HFIELD = 1, MJX_GEOM_SPHERE = 2, MJX_GEOM_CAPSULE = 3,
       MJX_GEOM_ELLIPSOID = 4, MJX_GEOM_CYLINDER = 5, MJX_GEOM_BOX = 6, MJX_GEOM_MESH = 7 };
/* joint types (mjtJoint) */
enum { MJX_JNT_FREE = 0, MJX_JNT_BALL = 1, MJX_JNT_SLIDE = 2, MJX_JNT_HINGE = 3 };
/* sensor types (subset of mjtSensor used by mjlab tasks) */
enum { MJX_SENS_GYRO = 0, MJX_SENS_VELOCIMETER = 1, MJX_SENS_ACCELEROMETER = 2,
       MJX_SENS_SUBTREEANGMOM = 3, MJX_SENS_CONTACT = 4, MJX_SENS_FRAMEPOS = 5,
       MJX_SENS_FRAMEQUAT = 6, MJX_SENS_JOINTPOS = 7, MJX_SENS_JOINTVEL = 8,
       /* Extended sensors: evaluated after the step by one small kernel of their own
        * (csrc/sensor_ext.hip) from the fields the step stores, as is every MJX_SENS_FRAMEQUAT,
        * every sensor with a ref frame and the cutoff of any sensor.  Frame sensors take the
        * object types BODY (the inertial frame: xipos, ximat), XBODY (xpos, xmat), GEOM and SITE,
        * for the object and for the optional ref frame (sensor_reftype / sensor_refid; reftype
        * MJX_OBJ_NONE: the world).  MJX_SENS_FRAMEPOS above stays the step kernels' own: site_xpos
        * of a SITE, xpos of a BODY or XBODY, no ref; MJX_SENS_FRAMEPOSX is the frame position of
        * any object type (BODY: xipos), with or without a ref. */
       MJX_SENS_FRAMEPOSX = 9, MJX_SENS_FRAMEXAXIS = 10, MJX_SENS_FRAMEYAXIS = 11,
       MJX_SENS_FRAMEZAXIS = 12, MJX_SENS_FRAMELINVEL = 13, MJX_SENS_FRAMEANGVEL = 14,
       MJX_SENS_FRAMELINACC = 15, MJX_SENS_FRAMEANGACC = 16, MJX_SENS_SUBTREECOM = 17,
       MJX_SENS_SUBTREELINVEL = 18, MJX_SENS_ACTUATORPOS = 19, MJX_SENS_ACTUATORVEL = 20,
       MJX_SENS_ACTUATORFRC = 21, MJX_SENS_JOINTACTUATORFRC = 22, MJX_SENS_COUNT = 23 };
/* object types for sensors (mjtObj numbering) */
enum { MJX_OBJ_NONE = 0, MJX_OBJ_BODY = 1, MJX_OBJ_XBODY = 2, MJX_OBJ_JOINT = 3,
       MJX_OBJ_GEOM = 5, MJX_OBJ_SITE = 6, MJX_OBJ_ACTUATOR = 19 };
/* contact sensor reduce modes (sensor/contact_sensor.py:39-44) */
enum { MJX_REDUCE_NONE = 0, MJX_REDUCE_MINDIST = 1, MJX_REDUCE_MAXFORCE = 2,
       MJX_REDUCE_NETFORCE = 3 };
enum { MJX_INT_EULER = 0, MJX_INT_IMPLICITFAST = 1 };
/* equality types (mjtEq numbering); only MJX_EQ_JOINT is computed */
enum { MJX_EQ_CONNECT = 0, MJX_EQ_WELD = 1, MJX_EQ_JOINT = 2, MJX_EQ_TENDON = 3, MJX_EQ_FLEX = 4,
       MJX_EQ_DISTANCE = 5 };

/* Host-side compiled model (fp64 / int32).  Field names follow mjModel.  Array
 * widths per element are in the trailing comment.  Filled by the Python scene
 * compiler (mjlab-1_amd/mjlab_amd/compiler/model.py); consumed by mjx_model_create
 * (uploaded to HBM as fp32) and by the CPU oracle (oracle/oracle.c, fp64). */
typedef struct mjxModelDesc_ {
  int abi_version;
  int nq, nv, nu, nbody, njnt, ngeom, nsite, nsensor, nsensordata, npair;
  int nhfield, nhfielddata, nlevel;
  int nmaskword; /* 32-bit words per contact-sensor geom mask: ceil(ngeom / 32) */
  /* cone: 0 pyramidal, 1 elliptic (anything else is refused).  Elliptic: a contact of dimension
   * dim in {3, 4, 6} has dim constraint rows -- normal, two tangents, torsional, two rolling --
   * instead of the pyramid's 2 (dim - 1); nefc and every row counter (mjx_sim_stats) count
   * them, within the same capacities.  The outputs "contact_force" and "contact_torque" (and a
   * contact sensor's force / torque fields) are then the row forces themselves in the contact
   * frame: (f_0, f_1, f_2) and (f_3, f_4, f_5), zero below the dimension.  An elliptic model runs
   * the generic step kernels only. */
  int iterations, ls_iterations, integrator, cone;
  /* contact sensors: matches per sensor and world considered, the first contact_maxmatch in
   * contact order (>= 1; SimulationCfg.contact_sensor_maxmatch, sim/sim.py:95,141) */
  int contact_maxmatch;
  double timestep, tolerance, ls_tolerance, impratio, meaninertia;
  double gravity[3];
  /* bodies */
  const int32_t *body_parentid, *body_rootid, *body_weldid, *body_jntnum, *body_jntadr,
      *body_dofnum, *body_dofadr, *body_level, *body_childadr /* nbody+1 */,
      *body_child /* >=1 */, *body_mocapid;
  const double *body_pos /*3*/, *body_quat /*4*/, *body_ipos /*3*/, *body_iquat /*4*/,
      *body_mass, *body_inertia /*3*/, *body_subtreemass, *body_invweight0 /*2*/;
  const int32_t *level_start /* nlevel+1 */, *level_body /* nbody */;
  /* joints */
  const int32_t *jnt_type, *jnt_qposadr, *jnt_dofadr, *jnt_bodyid, *jnt_limited;
  const double *jnt_pos /*3*/, *jnt_axis /*3*/, *jnt_range /*2*/, *jnt_solref /*2*/,
      *jnt_solimp /*5*/, *jnt_margin, *jnt_stiffness;
  const double *qpos0 /* nq */, *qpos_spring /* nq */;
  /* dofs */
  const int32_t *dof_bodyid, *dof_jntid, *dof_parentid;
  const uint64_t *dof_bodymask; /* bit b set: dof is on the kinematic chain of body b */
  const double *dof_armature, *dof_damping, *dof_invweight0, *dof_frictionloss;
  /* geoms */
  const int32_t *geom_type, *geom_bodyid, *geom_contype, *geom_conaffinity, *geom_condim,
      *geom_priority, *geom_dataid;
  const double *geom_size /*3*/, *geom_pos /*3*/, *geom_quat /*4*/, *geom_friction /*3*/,
      *geom_solmix, *geom_solref /*2*/, *geom_solimp /*5*/, *geom_margin, *geom_gap,
      *geom_rbound;
  /* sites */
  const int32_t *site_bodyid;
  const double *site_pos /*3*/, *site_quat /*4*/;
  /* actuators (joint transmission, gain fixed, bias affine: <position>/<motor>) */
  const int32_t *actuator_trnid, *actuator_forcelimited, *actuator_ctrllimited;
  const double *actuator_gear, *actuator_gainprm /*3*/, *actuator_biasprm /*3*/,
      *actuator_forcerange /*2*/, *actuator_ctrlrange /*2*/;
  /* sensors */
  const int32_t *sensor_type, *sensor_objtype, *sensor_objid, *sensor_reftype, *sensor_refid,
      *sensor_adr, *sensor_dim, *sensor_intprm /*3*/;
  const uint32_t *sensor_geommask1 /*nmaskword*/, *sensor_geommask2 /*nmaskword*/;
  /* static broadphase: candidate geom pairs, geom1 has the lower geom type.  Pairs with a
   * static terrain geom (a heightfield, or a box on a body welded to the world) come last,
   * grouped by that geom: the engine culls them per geom block (terrain broadphase). */
  const int32_t *pair_geom1, *pair_geom2;
  /* heightfields */
  const int32_t *hfield_nrow, *hfield_ncol, *hfield_adr;
  const double *hfield_size /*4*/, *hfield_data /* nhfielddata, normalised [0,1] */;
  /* sensors, continued (appended: the fields above keep their offsets): cutoff > 0 clamps the
   * entries of a real-valued sensor to [-cutoff, cutoff]; quaternion and axis sensors and
   * contact sensors are never clamped */
  const double* sensor_cutoff;
  /* Equality constraints (appended).  Only joint equalities are computed (eq_type ==
   * MJX_EQ_JOINT, mjEQ_JOINT): eq_obj1id / eq_obj2id are hinge or slide joints (eq_obj2id -1:
   * none), eq_data[0..4] the polynomial coefficients; with d = qpos[j2] - qpos0[j2]
   *   pos = qpos[j1] - qpos0[j1] - (c0 + c1 d + c2 d^2 + c3 d^3 + c4 d^4),
   *   J[dof1] = 1, J[dof2] = -(c1 + 2 c2 d + 3 c3 d^2 + 4 c4 d^3), margin 0,
   * impedance and reference acceleration from eq_solref / eq_solimp by the rules of limits and
   * contacts.  The engine emits every equality with eq_active0 != 0 as two opposed one-sided
   * rows (+J, +pos) and (-J, -pos) ahead of the limit and contact rows: nefc, njmax and every
   * row counter (mjx_sim_stats) count TWO rows per active equality.  At most 64 equalities;
   * mjx_model_create refuses any other eq_type, ids out of range, ball or free joints and
   * obj1 == obj2; mjx_sim_create a row capacity below 2 neq.  Such a model runs the generic
   * kernels.  A host that leaves neq 0 leaves the pointers unread. */
  int neq;
  const int32_t *eq_type, *eq_obj1id, *eq_obj2id, *eq_active0;
  const double *eq_data /*5*/, *eq_solref /*2*/, *eq_solimp /*5*/;
  /* Torsional and rolling friction (appended).  geom_condim is 1, 3, 4 or 6 (mjx_model_create
   * refuses any other): a contact of dimension dim > 1 has 2 (dim - 1) pyramid rows, pair k of
   * them J_n +/- mu_k J_k with mu = (f0, f0, f1, f2, f2) of the mixed geom_friction, J_0 / J_1
   * the relative linear velocity along the tangents, J_2 the relative angular velocity (body 2
   * minus body 1) along the normal and J_3 / J_4 along the tangents.  max_condim is the largest
   * geom_condim, or 0 to have it derived (any other value that is not the largest is refused).
   * A model with max_condim > 3 runs the generic kernels, its contacts count 2 (max_condim - 1)
   * rows in every capacity (mjx_sim_create_ex refuses an njmax_max below one such contact), and
   * the data field "contact_torque" [nworld, nconmax, 3] holds (torsional, rolling 1, rolling 2)
   * in the contact frame, zero for contacts of dimension <= 3. */
  int max_condim;
} mjxModelDesc;

size_t mjx_model_desc_size(void); /* sizeof(mjxModelDesc): ABI check for FFI bindings */

typedef struct mjxModel_ mjxModel; /* device-resident fp32 model (opaque) */
typedef struct mjxSim_ mjxSim;     /* nworld batched data + workspace (opaque) */

const char* mjx_last_error(void);
int mjx_abi_version(void);

/* Upload a compiled model to HBM (fp32).  `device` = HIP device ordinal. */
int mjx_model_create(const mjxModelDesc* desc, int device, mjxModel** out);
int mjx_model_destroy(mjxModel* model);

/* Allocate batched data for `nworld` worlds.  nconmax: contacts per world (the
 * reference's per-world budget, sim/sim.py:82-92); njmax: constraint rows per world.
 * Data starts at qpos0 (mj_resetData semantics). */
int mjx_sim_create(const mjxModel* model, int nworld, int nconmax, int njmax, mjxSim** out);
/* The same with a max capacity (nconmax <= 64, nconmax <= nconmax_max <= 512, njmax <=
 * njmax_max, and njmax_max >= nconmax_max past 64 contacts: every contact makes a row, so the
 * reference's njmax bounds a world's contacts too): the step
 * runs at (nconmax, njmax) per world -- the fast LDS carve -- and a world whose contacts or
 * rows overflow it in a substep is re-solved at (nconmax_max, njmax_max) instead of
 * truncated (the reference's budget semantics: its nconmax is pooled, sim/sim.py:82-92; its
 * njmax, 300 rows for the velocity tasks, bounds each world).  Only what overflows the max
 * capacity is dropped (counted by mjx_sim_stats).  The contact output arrays hold
 * nconmax_max slots per world; a masked forward re-solves its overflowing worlds too.  A batch
 * the engine splits into concurrent halves (large batches of models without Newton row
 * classes) re-solves behind each half's launches; only a split forced onto a model with row
 * classes (MJX355_SPLIT, diagnostic) keeps the fast carve as its max capacity (mjx_sim_info
 * reports the capacity wired). */
int mjx_sim_create_ex(const mjxModel* model, int nworld, int nconmax, int njmax, int nconmax_max,
                      int njmax_max, mjxSim** out);
int mjx_sim_destroy(mjxSim* sim);

/* One mj_step (forward + implicitfast/Euler integration) for every world, repeated
 * `nsubstep` times (ctrl/xfrc/qfrc_applied held fixed).  The state (qpos, qvel, act, time,
 * qacc_warmstart) advances every substep; the derived mjData outputs -- frames, contacts,
 * forces, subtree momenta and sensordata -- are the last substep's, computed in that substep
 * only (the contact sensors run every substep: the contact air times read their counts). */
int mjx_step(mjxSim* sim, int nsubstep, void* stream);
/* mj_forward without integration (kinematics/sensors/acc for the current state). */
int mjx_forward(mjxSim* sim, void* stream);
/* mj_forward only on worlds where mask[w] != 0 (mask: device uint8[nworld]; NULL = all).
 * Lets a sync-free (graph-captured) env step refresh just the worlds it reset. */
int mjx_forward_masked(mjxSim* sim, const uint8_t* mask, void* stream);
/* mj_resetData on worlds where mask[w] != 0 (mask: device uint8[nworld]; NULL = all). */
int mjx_reset(mjxSim* sim, const uint8_t* mask, void* stream);

/* Field access.  Data fields have a leading nworld dimension; model fields a
 * leading dimension of 1 (shared, world stride 0) or nworld after expansion.
 * The returned DLManagedTensor aliases library memory (float32/int32 on the sim's
 * device); call its deleter when done.  Pointers are stable for the sim's
 * lifetime except that mjx_expand_field reallocates that model field. */
struct DLManagedTensor;
int mjx_field(mjxSim* sim, const char* name, struct DLManagedTensor** out);
int mjx_field_count(const mjxSim* sim);
const char* mjx_field_name(const mjxSim* sim, int i);
int mjx_expand_field(mjxSim* sim, const char* name, void* stream);
int mjx_field_is_expanded(const mjxSim* sim, const char* name);

/* Contact-sensor air-time tracking inside the step (ContactSensor._update_air_time_tracking,
 * sensor/contact_sensor.py:327-367): after every integrated substep, for each of the `n`
 * tracked slots (n <= 8) with its `found` value at sensordata[found_adr[i]], update the
 * device buffers cur_air / last_air / cur_contact / last_contact [nworld, n] with the
 * elapsed time = time - last_time[w], then last_time[w] = time.  mjx_forward does not
 * update them.  found_adr is a host array; n = 0 turns tracking off.  Synchronises. */
int mjx_sim_track_air_time(mjxSim* sim, int n, const int32_t* found_adr, float* cur_air,
                           float* last_air, float* cur_contact, float* last_contact,
                           float* last_time, void* stream);

/* Explicit actuators inside the step (mjlab_amd/actuator.py: IdealPdActuator,
 * DcMotorActuator, DelayedActuator).  Actuator u with kind[u] != 0 is a <motor> whose ctrl
 * the engine computes every substep, in phase A, from the joint's position q and velocity qd
 * of that substep:
 *   t = kp (pt - q);  t += kd (vt - qd);  t += ft;
 *   kind 2 (ideal PD): ctrl = clamp(t, -effort_limit, effort_limit)
 *   kind 3 (DC motor): r = clamp(qd, -corner_velocity, corner_velocity) / velocity_limit,
 *     ctrl = clamp(t, max(saturation_effort (-1 - r), -effort_limit),
 *                     min(saturation_effort (1 - r), effort_limit))
 *   kind 1 (delayed builtin): ctrl = pt, the position target itself (read late, below),
 *     which the model's own position / velocity / motor actuator then takes
 * every operation rounded once, in this order (the torch form computes the same bits).  The
 * model's ctrlrange / forcerange then apply as to any ctrl, and the last substep of a step
 * (and a forward) stores the value in data.ctrl.  Kind 0 actuators take data.ctrl as before.
 * With max_lag[u] > 0 the position target is read `lag` substeps late: lag = min(lag[w,u],
 * frames pushed since the reset); lag 0 reads position_target, lag k > 0 frame ring_len - k
 * of the ring.  After every integrated substep (not in a forward) the engine shifts the ring,
 * appends position_target, counts the push (pushes[w,u], saturating at ring_len) and, where
 * min_lag[u] < max_lag[u] and hold[w,u] is zero, draws the next substep's lag uniformly on [min_lag, max_lag] from
 * a hash of (seed, w, group[u], draws[w,u]++): the actuators of a group share their lags.
 * A reset of a world is the caller's: zero its pushes and hold (and set its lag); draws is never
 * cleared.  The host tables are copied; the device buffers stay the caller's (float or int32,
 * [nworld, nu] unless noted), are read at every step, and must outlive the binding -- writing
 * them (gains, limits, lags) acts on the next step without another call.  A null descriptor
 * turns the explicit actuators off.  Synchronises. */
typedef struct mjxActuatorDesc {
  int32_t nworld, nu;
  int32_t ring_len;          /* frames per world of `ring`, <= 32; 0 when nothing is delayed */
  int32_t reserved;
  const uint8_t* kind;       /* host [nu]: 0 builtin, 1 delayed builtin, 2 ideal PD, 3 DC motor */
  const uint8_t* min_lag;    /* host [nu], substeps */
  const uint8_t* max_lag;    /* host [nu], <= ring_len; 0: not delayed */
  const uint8_t* group;      /* host [nu] */
  uint64_t seed;
  const float *kp, *kd, *effort_limit;
  const float *saturation_effort, *velocity_limit, *corner_velocity; /* kind 3 only */
  const float *position_target, *velocity_target, *effort_target;
  float* ring;               /* [nworld, ring_len, nu], oldest frame first */
  int32_t *lag, *pushes, *draws;
  const int32_t* hold;       /* nonzero: the lag is pinned, no draw replaces it; may be null */
} mjxActuatorDesc;
size_t mjx_actuator_desc_size(void);
int mjx_sim_set_actuators(mjxSim* sim, const mjxActuatorDesc* desc, void* stream);

/* Learned actuators (mjlab_amd/actuator.py: LearnedMlpActuator), bound after
 * mjx_sim_set_actuators.  Actuator u with net[u] != 255 must be of kind 3 there (a DC motor,
 * its kp and kd unused): its PD term t is replaced by the output of MLP net[u] on the last
 * `history` frames (e, v) = (pt - q, qd) of its joint -- the current substep's (pt read late as
 * for any delayed actuator) and history - 1 before it:
 *   input = [e_0 .. e_{H-1} | v_0 .. v_{H-1}], e scaled by pos_scale, v by vel_scale, index =
 *   lag; input_order 1 puts the velocities first.  A lag is clamped to the frames pushed since
 *   the reset; with none pushed every lag reads the current frame.
 *   x <- activation_l(W_l x + b_l) for l < nlayer (fp32, fused multiply-adds);
 *   t = x[0] * torque_scale, then the kind-3 clip above.
 * width[l] / width[l + 1] are layer l's input / output widths: width[0] = 2 * history, every
 * width <= 32, width[nlayer] = 1; activation[l]: 0 none, 1 relu, 2 softsign, 3 tanh, 4 elu
 * (alpha 1), none after the last layer.  weight[l] is host [width[l + 1], width[l]] row-major,
 * bias[l] host [width[l + 1]]: copied into device memory the sim owns (freed on the next
 * binding, a null descriptor, mjx_sim_set_actuators and mjx_sim_destroy).
 * history [nworld, hist_len, 2, nu] (hist_len = the largest history - 1; frames oldest first,
 * e then v), staging [nworld, 2, nu] and pushes [nworld, nu] are device buffers of the
 * caller's: phase A stores the frame it used in staging, and every integrated substep (not a
 * forward) shifts an actuator's last history - 1 frames by one, appends the staged frame and
 * counts the push, saturating at history - 1.  A reset of a world is the caller's: zero its
 * pushes.  With hist_len = 0 the three may be null.  Synchronises. */
#define MJX_MAX_ACT_NETS 4
#define MJX_MAX_NET_LAYERS 4
typedef struct mjxActuatorNet {
  int32_t nlayer;            /* 1..4 linear layers */
  int32_t history;           /* 1..8 frames */
  int32_t input_order;       /* 0: [pos | vel], 1: [vel | pos] */
  int32_t reserved;
  int32_t width[MJX_MAX_NET_LAYERS + 1];
  int32_t activation[MJX_MAX_NET_LAYERS];
  float pos_scale, vel_scale, torque_scale;
  const float* weight[MJX_MAX_NET_LAYERS];
  const float* bias[MJX_MAX_NET_LAYERS];
} mjxActuatorNet;
typedef struct mjxActuatorNetDesc {
  int32_t nworld, nu;
  int32_t nnet;              /* 1..4 */
  int32_t hist_len;          /* max over the networks of history - 1 */
  mjxActuatorNet nets[MJX_MAX_ACT_NETS];
  const uint8_t* net;        /* host [nu]: network of actuator u, 255: none */
  float* history;
  float* staging;
  int32_t* pushes;
} mjxActuatorNetDesc;
size_t mjx_actuator_net_desc_size(void);
int mjx_sim_set_actuator_nets(mjxSim* sim, const mjxActuatorNetDesc* desc, void* stream);

/* Diagnostics: per-sim counters as int32[8] written to host `out` ([0] max contacts, [1] max
 * rows seen, [2] contact-overflow, [3] row-overflow, [4] unsupported-pair events -- dropped
 * work --, [5] max Newton iterations, [6] worlds re-solved at the max capacity); synchronises
 * the stream. */
int mjx_sim_stats(mjxSim* sim, int32_t* out, void* stream);
/* The sim's capacities and kernels as int32[8]: [0] nconmax, [1] njmax (the fast carve),
 * [2] nconmax_max, [3] njmax_max, [4] spec of the fast carve's kernels, [5] spec of the max
 * capacity's kernels (csrc/specs.inc entry, 0 = generic), [6] re-solve list capacity per
 * substep, [7] Newton row classes. */
int mjx_sim_info(const mjxSim* sim, int32_t* out);
/* Diagnostics (parity tests): the joint-space inertia M of every world as the last substep's
 * phase A formed it (mjData.qM, mj_crb + armature; the reference reads it from mujoco_warp's
 * Data.qM), copied from the engine's phase hand-off scratch into the device buffer `out`:
 * float [nworld][L] with L = 8 nb (nb + 1), nb = ceil(nv / 4), the lower 4 x 4 tiles of the
 * nvp x nvp matrix row by row (row i = 4b + r holds columns [0, 4(b + 1)) at 8 b (b + 1) +
 * 4 (b + 1) r).  `big` = 1 reads the max-capacity scratch (worlds the overflow re-solve ran).
 * Valid after mjx_step / mjx_forward until the next launch; stream-ordered. */
int mjx_sim_mass_matrix(mjxSim* sim, int big, float* out, void* stream);
/* Diagnostics: per-stage cycle sums uint64[48] (non-zero only in the -DMJX_STAMPS build). */
int mjx_sim_profile(mjxSim* sim, uint64_t* out, void* stream);
/* Which step kernels the sim launches: k > 0 = kernels compiled for entry k of
 * csrc/specs.inc (the sim's dims, nconmax and njmax equal that entry), 0 = the generic
 * kernels; -1 for a null sim.  No reference counterpart (mujoco_warp specialises by
 * tracing Python at graph-capture time, sim/sim.py:164-191). */
int mjx_sim_spec(const mjxSim* sim);
/* Load a run-time specialisation: `path` is a shared library built from csrc/jit.hip for one
 * model's dims (mjlab_amd/jit.py compiles it with hipcc when a Simulation's model matches no
 * compiled csrc/specs.inc entry, and caches it).  Returns the specialisation id (>= 1000; a sim
 * created afterwards with those dims runs its kernels, mjx_sim_spec) or -1.  No reference
 * counterpart: mujoco_warp specialises kernels for any model by tracing at graph-capture
 * time (sim/sim.py:164-191); this is the AOT-compiled equivalent.  A library built from other
 * kernel headers than this engine (its mjx_jit_hdr differs from csrc/Makefile's MJX_HDR_HASH)
 * is refused (-1): its kernels would read the launch parameters through another layout. */
int mjx_spec_register(const char* path);
/* Diagnostics: enqueue one empty kernel (`mjx::marker_kernel`, one wave, argument `tag`) on
 * `stream`.  bench.py brackets its timed region with tags 1 and 2 outside the timing, so a
 * rocprofv3 kernel trace or --pmc pass of the same command can attribute exactly the
 * timed steps' dispatches.  No reference counterpart. */
int mjx_marker(int tag, void* stream);
/* Diagnostics (host side only): how many kernel launches of each kind this process has issued
 * through mjx_step / mjx_forward / mjx_forward_masked since it started or since the last
 * mjx_launch_counts_reset.  out[0..12] count the step-kernel entry points by phase code
 * (csrc/engine_impl.h phase_kernel), out[13] the Newton work-list kernel (classify); entries
 * past 13 are zeroed.  A launch captured into a graph counts once, at capture.  The tests use
 * it to show that a launch variant (a batch-size threshold or MJX355_* knob of
 * csrc/engine.hip launch_step) really ran.  Returns 0, or -1 for a null `out` or n < 0.  No
 * reference counterpart. */
int mjx_launch_counts(int64_t* out, int n);
int mjx_launch_counts_reset(void);
/* Diagnostics (host side only): launches of the extended-sensor kernel (MJX_SENS_FRAMEPOSX and
 * later, MJX_SENS_FRAMEQUAT, ref frames, cutoffs) this process has issued, written to out[0];
 * counted apart from mjx_launch_counts, whose layout is fixed, and cleared with them by
 * mjx_launch_counts_reset.  A model without extended sensors launches none; one with them
 * launches one per mjx_step / mjx_forward / mjx_forward_masked.  Returns 0, or -1 for a null
 * `out`.  No reference counterpart. */
int mjx_sensor_launch_count(int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MJX355_H_ */
