// model_tables.h — everything mjx_model_create derives from a model descriptor, on the host.
//
// build_model_tables holds every check of the descriptor and all the arithmetic between the
// descriptor and the device tables of engine.h DModel; it makes no HIP runtime call, so it runs
// (and is tested, tests/test_model_tables.py) without a GPU, and capi.cpp calls it before it
// touches a device.  capi.cpp uploads the vectors as they are; an empty one becomes one zeroed
// element there (capi.cpp upload), not here.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mjx355.h"
#include "engine.h"

namespace mjx {

struct ModelTables {
  Dims d{};  // nconmax = njmax = 0: the sim sets its capacities
  Opt o{};
  int nmaskword = 0;
  int neq = 0;     // joint equalities (fields.h counts the eq_* fields by it)
  int max_condim = 3;  // largest geom_condim, at least 3 (check_condims; engine.h DModel::max_condim)
  int ncsens = 0;  // 0 past 64 single-slot contact sensors (phase C then matches serially)
  std::vector<int32_t> dof_parentid;  // as given: find_spec checks a specialisation's dof tree
  // engine.h DModel, the host-derived part
  std::vector<uint64_t> dof_ancmask, body_submask, body_dofmask;
  std::vector<int32_t> body_rec, dof_rec, act_rec;
  std::vector<int32_t> geom_lds, lds_geom;
  std::vector<int32_t> st_geom, st_pairadr, st_partner;
  std::vector<float> st_aabb, st_chunk_aabb;
  std::vector<int32_t> pair_rec;  // empty: the ids exceed the packing, or no regular pair
  std::vector<int32_t> cs_sensor;
  std::vector<uint64_t> geom_csmask1, geom_csmask2;
  // static terrain geoms (heightfields, boxes welded to the world) and their world frames,
  // which the sim writes once into every world's geom_xpos / geom_xmat
  std::vector<int32_t> static_geoms;
  std::vector<float> static_xpos, static_xmat;
  std::vector<SensorExtRec> sensor_ext;  // engine.h SensorExtRec, sorted by kind
};

namespace tables {

inline bool is_static(const mjxModelDesc& desc, int g) {
  const int t = desc.geom_type[g];
  return t == GEOM_HFIELD || (t == GEOM_BOX && desc.body_weldid[desc.geom_bodyid[g]] == 0);
}

// The engine's size limits, and the lanes of the trees' roots.
inline std::string check_limits(const mjxModelDesc& desc) {
  if (desc.abi_version != MJX_ABI_VERSION) return "ABI version mismatch";
  if (desc.nbody > kMaxBodies) return "at most 64 bodies per world supported";
  if (desc.nv > kMaxDof) return "at most 64 dofs per world supported";
  // Phase B holds M and the Newton Hessian as two 4x4 register tiles per lane (engine_impl.h
  // Tiles): 128 tiles, the lower triangle of 60 padded dofs.  64 padded dofs have 136, and the
  // step would drop the last eight.
  if (desc.nv > 60)
    return "at most 60 dofs per world supported (61 to 64 need a third register tile per lane)";
  // Phase A moves a tree's frames back to the world with a lane shuffle indexed by the root's
  // body id, while lanes hold bodies in level order (level_body): the lane read must hold the
  // root itself, or, for a root that is not free, any body that is not free (both add zero).
  if (desc.nbody > 0 && desc.level_body && desc.body_rootid) {
    auto is_free = [&](int b) {
      return desc.body_jntnum[b] > 0 && desc.jnt_type[desc.body_jntadr[b]] == 0;
    };
    for (int b = 1; b < desc.nbody; b++) {
      const int r = desc.body_rootid[b];
      if (r < 0 || r >= desc.nbody) return "body_rootid out of range";
      const int x = desc.level_body[r];
      if (x != r && (is_free(r) || is_free(x)))
        return "a tree that follows a tree of several bodies is not supported: its root's "
               "body id is not its level-order lane (one articulated tree, then single bodies)";
    }
  }
  if (desc.nu > kMaxLanes || desc.njnt > kMaxLanes)
    return "at most 64 actuators and 64 joints per world supported";
  if (desc.cone != 0 && desc.cone != 1)
    return "cone " + std::to_string(desc.cone) + " is not supported (0 pyramidal, 1 elliptic)";
  if (desc.contact_maxmatch < 1) return "contact_maxmatch must be >= 1";
  return "";
}

// The extended-sensor table (engine.h SensorExtRec), sorted by kind, every id checked against
// the model's sizes: a bad id is an error here, not a device fault.
inline std::string build_sensor_ext(const mjxModelDesc& desc, std::vector<SensorExtRec>& out) {
  auto frame_ok = [&](int type, int id) {
    const int n = type == OBJ_BODY || type == OBJ_XBODY ? desc.nbody
                  : type == OBJ_GEOM ? desc.ngeom : type == OBJ_SITE ? desc.nsite : -1;
    return id >= 0 && id < n;
  };
  auto frame_body = [&](int type, int id) {
    return type == OBJ_GEOM ? desc.geom_bodyid[id] : type == OBJ_SITE ? desc.site_bodyid[id] : id;
  };
  for (int s = 0; s < desc.nsensor; s++) {
    const int type = desc.sensor_type[s], ot = desc.sensor_objtype[s], oi = desc.sensor_objid[s];
    const int rt = desc.sensor_reftype[s], ri = desc.sensor_refid[s];
    const int adr = desc.sensor_adr[s], dim = desc.sensor_dim[s];
    // (a host that leaves the appended sensor_cutoff null has no cutoffs)
    const float cutoff = desc.sensor_cutoff ? (float)desc.sensor_cutoff[s] : 0.f;
    const std::string who = "sensor " + std::to_string(s) + ": ";
    if (type < 0 || type >= SENS_COUNT) return who + "unknown sensor type " + std::to_string(type);
    if (adr < 0 || dim < 0 || adr + dim > desc.nsensordata) return who + "sensordata range out of bounds";
    if (type == SENS_CONTACT) continue;
    const bool frame = type == SENS_FRAMEQUAT || (type >= SENS_FRAMEPOSX && type <= SENS_FRAMEANGACC);
    if (type == SENS_FRAMEPOS && rt != OBJ_NONE)
      return who + "MJX_SENS_FRAMEPOS takes no ref frame (MJX_SENS_FRAMEPOSX does)";
    SensorExtRec r{};
    r.kind = type; r.adr = adr; r.dim = dim; r.cutoff = cutoff > 0.f ? cutoff : 0.f;
    r.otype = ot; r.oid = oi; r.rtype = OBJ_NONE;
    if (frame) {
      if (dim != (type == SENS_FRAMEQUAT ? 4 : 3)) return who + "frame sensor dimension";
      if (!frame_ok(ot, oi)) return who + "object type or id out of range";
      r.obody = frame_body(ot, oi);
      if (r.obody < 0 || r.obody >= desc.nbody) return who + "object body id out of range";
      r.oroot = desc.body_rootid[r.obody];
      if (rt != OBJ_NONE) {
        if (type == SENS_FRAMELINACC || type == SENS_FRAMEANGACC)
          return who + "framelinacc / frameangacc take no ref frame";
        if (!frame_ok(rt, ri)) return who + "ref type or id out of range";
        r.rtype = rt; r.rid = ri; r.rbody = frame_body(rt, ri);
        if (r.rbody < 0 || r.rbody >= desc.nbody) return who + "ref body id out of range";
        r.rroot = desc.body_rootid[r.rbody];
        if (r.rroot < 0 || r.rroot >= desc.nbody) return who + "ref root id out of range";
      }
      if (r.oroot < 0 || r.oroot >= desc.nbody) return who + "object root id out of range";
      if (type == SENS_FRAMEQUAT || (type >= SENS_FRAMEXAXIS && type <= SENS_FRAMEZAXIS)) r.cutoff = 0.f;
    } else if (type >= SENS_SUBTREECOM) {
      const bool body = type == SENS_SUBTREECOM || type == SENS_SUBTREELINVEL;
      const int n = body ? desc.nbody : type == SENS_JOINTACTUATORFRC ? desc.njnt : desc.nu;
      if (oi < 0 || oi >= n) return who + "object id out of range";
      if (dim != (body ? 3 : 1)) return who + "sensor dimension";
      if (type == SENS_JOINTACTUATORFRC) {
        const int jt = desc.jnt_type[oi];
        if (jt != JNT_HINGE && jt != JNT_SLIDE) return who + "jointactuatorfrc takes a hinge or slide joint";
        r.oid = desc.jnt_dofadr[oi];  // the entry of qfrc_actuator
        if (r.oid < 0 || r.oid >= desc.nv) return who + "joint dof address out of range";
      }
    } else {
      // a kind the step kernels write: listed only for its cutoff
      if (r.cutoff <= 0.f) continue;
      r.kind = kSensClamp;
    }
    out.push_back(r);
  }
  std::stable_sort(out.begin(), out.end(),
                   [](const SensorExtRec& a, const SensorExtRec& b) { return a.kind < b.kind; });
  if (out.size() > 65535) return "at most 65535 extended sensors (one grid row each)";
  return "";
}

// Joint equalities: the only kind the engine computes, every id checked here (phase A indexes
// jnt_* and qpos by them).
inline std::string check_equalities(const mjxModelDesc& desc) {
  if (desc.neq < 0) return "neq must not be negative";
  if (desc.neq > kMaxEq) return "at most 64 equality constraints per world supported";
  if (desc.neq > 0 && (!desc.eq_type || !desc.eq_obj1id || !desc.eq_obj2id || !desc.eq_active0 ||
                       !desc.eq_data || !desc.eq_solref || !desc.eq_solimp))
    return "neq > 0 with a null eq_* array";
  for (int e = 0; e < desc.neq; e++) {
    const std::string who = "equality " + std::to_string(e) + ": ";
    if (desc.eq_type[e] != MJX_EQ_JOINT)
      return who + "only joint equalities are supported (eq_type " + std::to_string(desc.eq_type[e]) + ")";
    const int j1 = desc.eq_obj1id[e], j2 = desc.eq_obj2id[e];
    if (j1 < 0 || j1 >= desc.njnt || j2 < -1 || j2 >= desc.njnt) return who + "joint id out of range";
    if (j1 == j2) return who + "joint1 and joint2 are the same joint";
    for (int j : {j1, j2})
      if (j >= 0 && desc.jnt_type[j] != JNT_HINGE && desc.jnt_type[j] != JNT_SLIDE)
        return who + "a joint equality takes hinge or slide joints";
  }
  return "";
}

// Contact dimensions: 1 (frictionless), 3 (sliding), 4 (+ torsional) and 6 (+ rolling) have rows;
// the descriptor's max_condim, where a host sets it, is the largest of them (0: derived here).
inline std::string check_condims(const mjxModelDesc& desc, int& max_condim) {
  max_condim = 3;
  for (int g = 0; g < desc.ngeom; g++) {
    const int cd = desc.geom_condim[g];
    if (cd != 1 && cd != 3 && cd != 4 && cd != 6)
      return "geom " + std::to_string(g) + ": condim " + std::to_string(cd) +
             " is not supported (1, 3, 4 or 6)";
    if (cd > max_condim) max_condim = cd;
  }
  if (desc.max_condim != 0 && std::max(desc.max_condim, 3) != max_condim)
    return "max_condim " + std::to_string(desc.max_condim) + " is not the largest geom_condim (" +
           std::to_string(max_condim) + ")";
  return "";
}

// Sizes and options as the kernels take them (npair .. nstpartner: terrain_tables).
inline void dims_and_options(const mjxModelDesc& desc, ModelTables& t) {
  Dims& d = t.d;
  d.nq = desc.nq; d.nv = desc.nv; d.nu = desc.nu; d.nbody = desc.nbody; d.njnt = desc.njnt;
  d.ngeom = desc.ngeom; d.nsite = desc.nsite; d.nsensor = desc.nsensor;
  d.nsensordata = desc.nsensordata; d.npair = desc.npair; d.nhfield = desc.nhfield;
  d.nhfielddata = desc.nhfielddata; d.nlevel = desc.nlevel;
  d.nchild = desc.body_childadr[desc.nbody];
  if (d.nchild < 1) d.nchild = 1;
  d.nmocap = 0;
  for (int b = 0; b < d.nbody; b++)
    if (desc.body_mocapid[b] >= 0) d.nmocap++;
  d.nconmax = 0; d.njmax = 0;
  t.neq = desc.neq;
  Opt& o = t.o;
  o.timestep = (float)desc.timestep; o.tolerance = (float)desc.tolerance;
  o.ls_tolerance = (float)desc.ls_tolerance; o.impratio = (float)desc.impratio;
  o.meaninertia = (float)desc.meaninertia;
  for (int i = 0; i < 3; i++) o.gravity[i] = (float)desc.gravity[i];
  o.iterations = desc.iterations; o.ls_iterations = desc.ls_iterations;
  o.integrator = desc.integrator; o.cone = desc.cone;
  o.maxmatch = desc.contact_maxmatch;
}

// Ancestor / subtree / dof masks and the per-lane records (engine.h DModel::body_rec).
inline void tree_tables(const mjxModelDesc& desc, ModelTables& t) {
  const int nv = desc.nv, nb = desc.nbody, nu = desc.nu;
  t.dof_parentid.assign(desc.dof_parentid, desc.dof_parentid + nv);
  // ancestor masks along dof_parentid (parents precede children in dof order)
  std::vector<uint64_t>& anc = t.dof_ancmask;
  anc.assign(nv, 0);
  for (int i = 0; i < nv; i++) {
    const int par = desc.dof_parentid[i];
    anc[i] = (1ull << i) | (par >= 0 && par < i ? anc[par] : 0ull);
  }
  // subtree masks (parents precede children in body order) and the dofs moving each body
  std::vector<uint64_t>&sub = t.body_submask, &bdof = t.body_dofmask;
  sub.assign(nb, 0);
  bdof.assign(nb, 0);
  for (int b = nb - 1; b >= 0; b--) {
    sub[b] |= 1ull << b;
    const int par = desc.body_parentid[b];
    if (b > 0 && par >= 0 && par < b) sub[par] |= sub[b];
  }
  for (int b = 0; b < nb; b++) {
    const int par = desc.body_parentid[b];
    if (b > 0 && par >= 0 && par < b) bdof[b] = bdof[par];
    for (int k = 0; k < desc.body_dofnum[b]; k++) bdof[b] |= 1ull << (desc.body_dofadr[b] + k);
  }
  // level-order bodies, dofs, actuators
  t.body_rec.assign((size_t)kBodyRec * nb, 0);
  for (int i = 0; i < nb; i++) {
    int32_t* r = t.body_rec.data() + (size_t)kBodyRec * i;
    const int b = desc.level_body[i];
    int lv = 0;
    for (int l = 1; l < desc.nlevel; l++) lv = i >= desc.level_start[l] ? l : lv;
    const int j0 = desc.body_jntadr[b], jn = desc.body_jntnum[b], k = jn > 0 ? j0 : 0;
    const int c0 = desc.body_childadr[b], cn = desc.body_childadr[b + 1] - c0;
    int chp = 0;
    for (int c = 0; c < 5 && c < cn; c++) chp |= desc.body_child[c0 + c] << (6 * c);
    const int32_t v[16] = {b, desc.body_parentid[b], lv, j0, jn, desc.jnt_type[k], desc.jnt_qposadr[k],
                           desc.jnt_dofadr[k], desc.body_dofadr[b], desc.body_dofnum[b],
                           desc.body_mocapid[b], desc.body_rootid[b], c0, cn, chp, 0};
    for (int c = 0; c < 16; c++) r[c] = v[c];
    r[16] = (int32_t)(uint32_t)sub[b]; r[17] = (int32_t)(uint32_t)(sub[b] >> 32);
    r[18] = (int32_t)(uint32_t)bdof[b]; r[19] = (int32_t)(uint32_t)(bdof[b] >> 32);
  }
  t.dof_rec.assign((size_t)kDofRec * nv, 0);
  for (int i = 0; i < nv; i++) {
    int32_t* r = t.dof_rec.data() + (size_t)kDofRec * i;
    const int j = desc.dof_jntid[i], body = desc.dof_bodyid[i];
    const int32_t v[8] = {body, desc.jnt_type[j], desc.jnt_qposadr[j], desc.body_parentid[body],
                          desc.jnt_dofadr[j], desc.body_dofadr[body], j, 0};
    for (int c = 0; c < 8; c++) r[c] = v[c];
    r[8] = (int32_t)(uint32_t)anc[i]; r[9] = (int32_t)(uint32_t)(anc[i] >> 32);
  }
  t.act_rec.assign((size_t)kActRec * nu, 0);
  for (int u = 0; u < nu; u++) {
    int32_t* r = t.act_rec.data() + (size_t)kActRec * u;
    const int j = desc.actuator_trnid[u];
    r[0] = desc.jnt_dofadr[j]; r[1] = desc.jnt_qposadr[j];
    r[2] = desc.actuator_ctrllimited[u]; r[3] = desc.actuator_forcelimited[u];
  }
}

// Terrain pair blocks.  The pair list is [regular pairs | terrain pairs], the terrain pairs
// grouped by their static terrain geom (the scene compiler emits them that way): a
// heightfield, or a box on a body welded to the world.  Those geoms keep no LDS frame.
inline std::string terrain_blocks(const mjxModelDesc& desc, ModelTables& t) {
  const int ng = desc.ngeom, np = desc.npair;
  Dims& d = t.d;
  t.geom_lds.assign(ng, -1);
  for (int g = 0; g < ng; g++)
    if (!is_static(desc, g)) { t.geom_lds[g] = (int)t.lds_geom.size(); t.lds_geom.push_back(g); }
  d.ngeom_lds = (int)t.lds_geom.size();
  int nreg = 0;
  while (nreg < np && !is_static(desc, desc.pair_geom1[nreg]) && !is_static(desc, desc.pair_geom2[nreg])) nreg++;
  std::vector<char> seen(ng, 0), done(ng, 0);
  for (int q = nreg; q < np; q++) {
    const int g1 = desc.pair_geom1[q], g2 = desc.pair_geom2[q];
    const bool s1 = is_static(desc, g1);
    if (s1 == is_static(desc, g2))
      return "pair list: terrain pairs (one static terrain geom each) must follow all regular pairs";
    const int sg = s1 ? g1 : g2, pg = s1 ? g2 : g1;
    if (desc.geom_type[sg] == GEOM_HFIELD ? sg != g1 : (sg != g2 && desc.geom_type[pg] != GEOM_BOX))
      return "pair list: a terrain pair must keep MuJoCo's geom-type order";
    if (t.st_geom.empty() || t.st_geom.back() != sg) {
      if (done[sg]) return "pair list: terrain pair blocks must be contiguous";
      done[sg] = 1;
      t.st_geom.push_back(sg);
      t.st_pairadr.push_back(q);
    }
    if (!seen[pg]) { seen[pg] = 1; t.st_partner.push_back(pg); }
  }
  t.st_pairadr.push_back(np);
  d.npair = nreg;
  d.npair_all = np;
  d.nboxbox = 0;
  for (int q = 0; q < np; q++)
    d.nboxbox += desc.geom_type[desc.pair_geom1[q]] == GEOM_BOX && desc.geom_type[desc.pair_geom2[q]] == GEOM_BOX;
  d.nstatic = (int)t.st_geom.size();
  d.nstpartner = (int)t.st_partner.size();
  return "";
}

// Static world frames of the terrain geoms (D.geom_xpos / geom_xmat), the AABBs of those with
// pairs (lo xyz, hi xyz, margin included) and their unions over chunks of kStaticChunk.
inline std::string terrain_frames(const mjxModelDesc& desc, ModelTables& t) {
  const int ng = desc.ngeom, nstatic = t.d.nstatic;
  std::vector<float>& aabb = t.st_aabb;
  aabb.assign((size_t)6 * nstatic, 0.f);
  std::vector<int> st_slot(ng, -1);
  for (int k = 0; k < nstatic; k++) st_slot[t.st_geom[k]] = k;
  for (int g = 0; g < ng; g++) {
    if (!is_static(desc, g)) continue;
    const int b = desc.geom_bodyid[g];
    if (desc.body_weldid[b] != 0) return "heightfield geoms must sit on bodies welded to the world";
    // chain of static bodies up to the world: x = x_parent + R_parent p, q = q_parent q
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, x[3] = {0, 0, 0};
    std::vector<int> chain;
    for (int c = b; c > 0; c = desc.body_parentid[c]) chain.push_back(c);
    auto qm = [](const double* q, double* M) {
      const double w = q[0], a = q[1], bq = q[2], c = q[3];
      M[0] = 1 - 2 * (bq * bq + c * c); M[1] = 2 * (a * bq - w * c); M[2] = 2 * (a * c + w * bq);
      M[3] = 2 * (a * bq + w * c); M[4] = 1 - 2 * (a * a + c * c); M[5] = 2 * (bq * c - w * a);
      M[6] = 2 * (a * c - w * bq); M[7] = 2 * (bq * c + w * a); M[8] = 1 - 2 * (a * a + bq * bq);
    };
    auto step = [&](const double* pos, const double* quat) {
      double Q[9], nx[3], nR[9];
      qm(quat, Q);
      for (int i = 0; i < 3; i++) nx[i] = x[i] + R[3 * i] * pos[0] + R[3 * i + 1] * pos[1] + R[3 * i + 2] * pos[2];
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
          nR[3 * i + j] = R[3 * i] * Q[j] + R[3 * i + 1] * Q[3 + j] + R[3 * i + 2] * Q[6 + j];
      for (int i = 0; i < 3; i++) x[i] = nx[i];
      for (int i = 0; i < 9; i++) R[i] = nR[i];
    };
    for (auto it = chain.rbegin(); it != chain.rend(); ++it)
      step(desc.body_pos + 3 * *it, desc.body_quat + 4 * *it);
    step(desc.geom_pos + 3 * g, desc.geom_quat + 4 * g);
    t.static_geoms.push_back(g);
    for (int i = 0; i < 3; i++) t.static_xpos.push_back((float)x[i]);
    for (int i = 0; i < 9; i++) t.static_xmat.push_back((float)R[i]);
    const int k = st_slot[g];
    if (k < 0) continue;
    // local box: a box's half sizes; a heightfield's [-sx, sx] x [-sy, sy] x [-base, zmax]
    double e[3], c[3] = {0, 0, 0};
    if (desc.geom_type[g] == GEOM_BOX) {
      for (int i = 0; i < 3; i++) e[i] = desc.geom_size[3 * g + i];
    } else {
      const double* hs = desc.hfield_size + 4 * desc.geom_dataid[g];
      e[0] = hs[0]; e[1] = hs[1]; e[2] = 0.5 * (hs[2] + hs[3]);
      c[2] = 0.5 * (hs[2] - hs[3]);
    }
    const double mg = desc.geom_margin[g];
    for (int i = 0; i < 3; i++) {
      const double cw = x[i] + R[3 * i] * c[0] + R[3 * i + 1] * c[1] + R[3 * i + 2] * c[2];
      const double hw = std::fabs(R[3 * i]) * e[0] + std::fabs(R[3 * i + 1]) * e[1] +
                        std::fabs(R[3 * i + 2]) * e[2] + mg;
      // rounded outward so the fp32 cull never rejects what the fp64 bounds admit
      aabb[6 * k + i] = std::nextafter((float)(cw - hw), -INFINITY);
      aabb[6 * k + 3 + i] = std::nextafter((float)(cw + hw), INFINITY);
    }
  }
  // (a model without terrain keeps one empty chunk: lo = +inf, hi = -inf)
  const int nchunk = std::max(1, (nstatic + kStaticChunk - 1) / kStaticChunk);
  t.st_chunk_aabb.resize((size_t)6 * nchunk);
  for (int c = 0; c < nchunk; c++) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = c * kStaticChunk; k < std::min(nstatic, (c + 1) * kStaticChunk); k++)
      for (int i = 0; i < 3; i++) {
        lo[i] = std::min(lo[i], aabb[6 * k + i]);
        hi[i] = std::max(hi[i], aabb[6 * k + 3 + i]);
      }
    for (int i = 0; i < 3; i++) { t.st_chunk_aabb[6 * c + i] = lo[i]; t.st_chunk_aabb[6 * c + 3 + i] = hi[i]; }
  }
  return "";
}

// Regular-pair records: the pair loop of phase A reads one coalesced 16-B record per lane
// instead of a chain of dependent per-geom loads (pair -> geom -> type / slot / margin /
// rbound); the cull radius is formed in fp32 exactly as the kernel forms it.
inline void pair_records(const mjxModelDesc& desc, ModelTables& t) {
  const int ng = desc.ngeom, nreg = t.d.npair;
  bool packable = ng < 65536 && t.d.ngeom_lds < 4096;
  for (int g = 0; g < ng && packable; g++) packable = desc.geom_type[g] >= 0 && desc.geom_type[g] < 16;
  if (!packable) return;
  std::vector<int32_t>& rec = t.pair_rec;
  rec.resize((size_t)4 * nreg);
  for (int q = 0; q < nreg; q++) {
    const int g1 = desc.pair_geom1[q], g2 = desc.pair_geom2[q];
    const int t1 = desc.geom_type[g1], t2 = desc.geom_type[g2];
    const float r1 = (float)desc.geom_rbound[g1], r2 = (float)desc.geom_rbound[g2];
    const float mg = std::fmax((float)desc.geom_margin[g1], (float)desc.geom_margin[g2]);
    const float cull = (r1 > 0 && r2 > 0 && t1 != GEOM_HFIELD) ? r1 + r2 + mg : INFINITY;
    rec[4 * q] = g1 | g2 << 16;
    rec[4 * q + 1] = t.geom_lds[g1] | t.geom_lds[g2] << 12 | t1 << 24 | (int32_t)((uint32_t)t2 << 28);
    std::memcpy(&rec[4 * q + 2], &mg, 4);
    std::memcpy(&rec[4 * q + 3], &cull, 4);
  }
}

// Transposed single-slot contact-sensor masks (engine.h geom_csmask1/2); more than 64 such
// sensors: ncsens = 0 and phase C matches sensor by sensor (serial path).
inline void contact_sensor_masks(const mjxModelDesc& desc, ModelTables& t) {
  std::vector<int32_t>& cs = t.cs_sensor;
  for (int s = 0; s < desc.nsensor; s++)
    if (desc.sensor_type[s] == SENS_CONTACT && desc.sensor_intprm[3 * s + 2] <= 1) cs.push_back(s);
  t.geom_csmask1.assign(desc.ngeom, 0);
  t.geom_csmask2.assign(desc.ngeom, 0);
  t.ncsens = cs.size() <= 64 ? (int)cs.size() : 0;
  for (int k = 0; k < t.ncsens; k++) {
    const uint32_t* a = desc.sensor_geommask1 + (size_t)desc.nmaskword * cs[k];
    const uint32_t* b = desc.sensor_geommask2 + (size_t)desc.nmaskword * cs[k];
    for (int g = 0; g < desc.ngeom; g++) {
      if ((a[g >> 5] >> (g & 31)) & 1u) t.geom_csmask1[g] |= 1ull << k;
      if ((b[g >> 5] >> (g & 31)) & 1u) t.geom_csmask2[g] |= 1ull << k;
    }
  }
}

}  // namespace tables

// Fills `t` (a fresh ModelTables) from the descriptor.  Returns "" or the refusal.
inline std::string build_model_tables(const mjxModelDesc& desc, ModelTables& t) {
  std::string err = tables::check_limits(desc);
  if (err.empty()) err = tables::check_equalities(desc);
  if (err.empty()) err = tables::check_condims(desc, t.max_condim);
  if (err.empty()) err = tables::build_sensor_ext(desc, t.sensor_ext);
  if (err.empty() && desc.nmaskword < (desc.ngeom + 31) / 32) err = "nmaskword < ceil(ngeom / 32)";
  if (!err.empty()) return err;
  t.nmaskword = desc.nmaskword;
  tables::dims_and_options(desc, t);
  tables::tree_tables(desc, t);
  err = tables::terrain_blocks(desc, t);
  if (err.empty()) err = tables::terrain_frames(desc, t);
  if (!err.empty()) return err;
  tables::pair_records(desc, t);
  tables::contact_sensor_masks(desc, t);
  return "";
}

}  // namespace mjx
