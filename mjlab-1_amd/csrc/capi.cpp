// capi.cpp — the extern "C" boundary declared in include/mjx355.h.
//
// Owns every device buffer (model blob, per-field data arrays, stats), hands out
// DLPack aliases, and enqueues the engine kernels on the caller's HIP stream.  The
// Python host mirror of mjlab.sim.Simulation (mjlab_amd/sim/sim.py) binds this with
// ctypes; INTEGRATION.md shows the same binding for other hosts.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <algorithm>
#include <vector>

#include "../../include/mjx355.h"
#include "engine.h"
#include "model_tables.h"

// ---------------------------------------------------------------- minimal DLPack ABI
extern "C" {
typedef struct { int32_t device_type; int32_t device_id; } DLDevice;
typedef struct { uint8_t code; uint8_t bits; uint16_t lanes; } DLDataType;
typedef struct {
  void* data;
  DLDevice device;
  int32_t ndim;
  DLDataType dtype;
  int64_t* shape;
  int64_t* strides;
  uint64_t byte_offset;
} DLTensor;
struct DLManagedTensor {
  DLTensor dl_tensor;
  void* manager_ctx;
  void (*deleter)(struct DLManagedTensor*);
};
}
static const int32_t kDLROCM = 10;

namespace {
thread_local std::string g_err;
int fail(const std::string& msg) {
  g_err = msg;
  return -1;
}
#define HIPCHK(expr)                                                                 \
  do {                                                                               \
    hipError_t e_ = (expr);                                                          \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct FieldInfo {
  void* ptr;
  bool is_float;
  int64_t count, width;
  bool per_world;     // data field (leading nworld) or expanded model field
  bool model;
  bool scalar = false;  // one value per world (time, ncon, ...): shape [nworld]
};
}  // namespace

// Ownership: a handle frees what it owns in its destructor, and nothing else frees it.  The
// create functions hold the handle in a std::unique_ptr until they succeed, so a failure at
// any point is a plain `return fail(...)`.
struct mjxModel_ {
  int device = 0;
  mjx::ModelTables t;  // host side: dims, options, dof tree, static terrain frames, tables
  mjx::DModel dm{};
  mjx::SensorExt ext;  // extended sensors (sensor_ext.hip); n = 0: the kernel is never launched
  std::vector<void*> allocs;  // every device buffer dm and ext point to
  // host fp32 copies of float fields (defaults for expansion)
  std::map<std::string, std::vector<float>> host_float;
  std::map<std::string, std::pair<int64_t, int64_t>> float_dims;  // count, width
  std::map<std::string, std::pair<int64_t, int64_t>> int_dims;
  ~mjxModel_() {
    for (void* p : allocs) (void)hipFree(p);
  }
};

// One contact / row capacity of a sim: its dims, phase carves, kernels and hand-off scratch.
struct Capacity {
  mjx::Dims d{};
  mjx::Lds lds[3]{};  // phases A, B (full row capacity), C
  int spec = 0;       // model specialisation in use (mjx::find_spec), 0 = generic kernels
  int gC = 0, gF = 0, gstride = 0;  // Params::gC / gF / gstride
  float* gscr = nullptr;
  mjx::Params* dparams = nullptr;  // device copy of the launch parameters
};

// The host part of a capacity; `too_big` is the refusal of a carve past a CU's LDS.
static int make_capacity(const mjx::Dims& d, const std::vector<int32_t>& dof_parentid, int neq,
                         int max_condim, int cone, const char* too_big, Capacity& c) {
  c.d = d;
  for (int i = 0; i < 3; i++) {
    // (phases A and C hold the contacts' friction coefficients: five each with torsional or
    // rolling contacts in the model)
    // (and an elliptic model's row slots carry the contact grouping: carve.h make_lds)
    c.lds[i] = mjx::make_lds(d, i, false, mjx::con_mu_width(max_condim), cone);
    if ((size_t)c.lds[i].total * 4 > 160 * 1024) return fail(too_big);
  }
  // a model with joint equalities runs the generic kernels: no specialisation holds the
  // equality rows' code (engine_impl.h neq_of), and none the rotational contact rows' (condim_of)
  // ... and none the elliptic cone's rows and solver (cone_of)
  c.spec = neq > 0 || max_condim > 3 || cone != 0 ? 0 : mjx::find_spec(d, dof_parentid.data());
  c.gC = (c.lds[1].pack_len + 63) & ~63;
  c.gF = c.gC + ((c.lds[2].pack_len + 63) & ~63);
  c.gstride = c.gF + ((mjx::ltr_size((d.nv + 3) & ~3) + 63) & ~63);  // implicit factor, LTR form
  return 0;
}

struct mjxSim_ {
  const mjxModel_* model = nullptr;
  int nworld = 0;
  mjx::DModel dm{};  // per-sim copy: expanded fields point to per-world buffers
  mjx::DData dd{};
  // the fast capacity, and the max capacity of the overflow re-solve (mjx_sim_create_ex with a
  // max capacity above the fast carve; valid when has_big)
  Capacity fast, big;
  bool has_big = false;
  // the launch parameters as sync_params last uploaded them (host_big: when has_big)
  mjx::Params host{}, host_big{};
  mjx::Lds lds_class[mjx::kRowClasses]{};  // phase B carve of Newton row class k
  int nrowclass = 0;
  int row_cap[mjx::kRowClasses] = {};
  int nair = 0;  // contact air-time tracking (mjx_sim_track_air_time)
  int air_found[mjx::kMaxAirSlots] = {};
  float* air_buf[5] = {};
  bool act_on = false;  // explicit actuators (mjx_sim_set_actuators)
  mjx::ActParams act{};
  mjx::NetParams net{};   // learned actuators (mjx_sim_set_actuator_nets)
  float* netw = nullptr;  // packed actuator-network weights (mjx_sim_set_actuator_nets)
  mjx::SideStream side{};  // streams of the Newton row classes (when classes are used)
  int* wl = nullptr;  // Newton work lists: [nworld] world ids + [kMaxSplit][2 * (kRowClasses + 1)] segments
  void* arena = nullptr;
  int* ovf = nullptr;  // the lists phase A fills for the re-solve: [kMaxSplit][2][ovf_cap] lists,
                       // [kMaxSplit][2] counts, [nworld] flags, [kMaxSplit][2] done counters
  int ovf_cap = 0;
  int con_stride = 0;  // contact slots per world in the contact output arrays
  std::vector<void*> expanded_allocs;
  std::map<std::string, FieldInfo> fields;
  std::vector<std::string> names;
  mjxSim_() {
    for (int u = 0; u < mjx::kWave; u++) net.net_of[u] = mjx::kNoNet;  // as drop_actuator_nets leaves it
  }
  ~mjxSim_() {
    for (int p = 0; p < mjx::kMaxSplit; p++) {
      if (side.fork[p]) (void)hipEventDestroy(side.fork[p]);
      for (int k = 0; k < mjx::kRowClasses; k++) {
        if (side.join[p][k]) (void)hipEventDestroy(side.join[p][k]);
        if (side.stream[p][k]) (void)hipStreamDestroy(side.stream[p][k]);
      }
    }
    for (int p = 0; p < mjx::kMaxSplit; p++) {
      if (side.split[p]) (void)hipStreamDestroy(side.split[p]);
      if (side.split_join[p]) (void)hipEventDestroy(side.split_join[p]);
    }
    if (side.split_fork) (void)hipEventDestroy(side.split_fork);
    for (int p = 0; p < mjx::kMaxSplit; p++) {
      if (side.ovf[p]) (void)hipStreamDestroy(side.ovf[p]);
      if (side.ovf_fork[p]) (void)hipEventDestroy(side.ovf_fork[p]);
      if (side.ovf_join[p]) (void)hipEventDestroy(side.ovf_join[p]);
    }
    for (void* p : {(void*)arena, (void*)wl, (void*)ovf, (void*)netw, (void*)fast.gscr,
                    (void*)fast.dparams, (void*)big.gscr, (void*)big.dparams})
      if (p) (void)hipFree(p);
    for (void* p : expanded_allocs) (void)hipFree(p);
  }
};

// The launch parameters of one capacity.  The max capacity (`max`) shares the model, data,
// lists and air-time buffers; it has no row classes (its worlds run the latency Newton
// kernel), and overflow past it drops contacts.
static mjx::Params host_params(const mjxSim_* s, const Capacity& c, bool max) {
  mjx::Params p;
  p.d = c.d;
  p.o = s->model->t.o;
  p.m = s->dm;
  p.D = s->dd;
  for (int i = 0; i < 3; i++) p.LP[i] = c.lds[i];
  for (int k = 0; k < mjx::kRowClasses; k++) p.LP[3 + k] = max ? c.lds[1] : s->lds_class[k];
  p.LPJ = mjx::make_lds(c.d, 1, true, 2, p.o.cone);
  p.nrowclass = max ? 0 : s->nrowclass;
  for (int k = 0; k < mjx::kRowClasses; k++) p.row_cap[k] = s->row_cap[k];
  p.gscr = c.gscr;
  p.wl_list = s->wl;
  p.wl_seg = s->wl ? s->wl + s->nworld : nullptr;
  p.gC = c.gC;
  p.gF = c.gF;
  p.gstride = c.gstride;
  p.spec = c.spec;
  p.nair = s->nair;
  for (int i = 0; i < mjx::kMaxAirSlots; i++) p.air_found[i] = s->air_found[i];
  p.air_cur = s->air_buf[0]; p.air_last = s->air_buf[1]; p.air_cc = s->air_buf[2];
  p.air_lc = s->air_buf[3]; p.air_time = s->air_buf[4];
  p.act_on = s->act_on ? 1 : 0;
  p.act = s->act;
  p.net = s->net;
  static const int minrows = [] {
    const char* e = getenv("MJX355_STAMP_MINROWS");
    return e ? atoi(e) : 0;
  }();
  p.stamp_minrows = minrows;
  static const int outputs_every = [] {
    const char* e = getenv("MJX355_OUTPUTS_EVERY");
    return e ? atoi(e) : 0;
  }();
  p.outputs_every = outputs_every;
  p.ovf_resolve = s->has_big && !max ? 1 : 0;
  p.ovf_cap = s->ovf_cap;
  p.ovf_list = s->ovf;
  p.ovf_n = s->ovf ? s->ovf + (size_t)mjx::kMaxSplit * 2 * s->ovf_cap : nullptr;
  p.ovf_flag = s->ovf ? p.ovf_n + mjx::kMaxSplit * 2 : nullptr;
  p.ovf_done = s->ovf ? p.ovf_flag + s->nworld : nullptr;
  p.con_stride = s->con_stride;
  return p;
}

// Rebuild the launch parameters from the sim's state and upload them (stream-ordered, so
// later launches see the new copy).  Every launch reads s->host / s->host_big: what the
// host uses for the launch geometry is what the device holds.
static int sync_params(mjxSim_* s, void* stream) {
  s->host = host_params(s, s->fast, false);
  HIPCHK(hipMemcpyAsync(s->fast.dparams, &s->host, sizeof(mjx::Params), hipMemcpyHostToDevice,
                        (hipStream_t)stream));
  if (s->has_big) {
    s->host_big = host_params(s, s->big, true);
    HIPCHK(hipMemcpyAsync(s->big.dparams, &s->host_big, sizeof(mjx::Params), hipMemcpyHostToDevice,
                          (hipStream_t)stream));
  }
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

// Upload a table into a buffer the model owns.  An empty table (or one shorter than `pad`
// elements) is padded with zeros: no model pointer is null or dangling.
template <class T>
static int upload(mjxModel_* m, const std::vector<T>& v, const T*& dst, size_t pad = 1) {
  const size_t n = std::max(v.size(), pad);
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, n * sizeof(T)));
  m->allocs.push_back(p);
  if (v.size() < n) HIPCHK(hipMemset(p, 0, n * sizeof(T)));
  if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  dst = (const T*)p;
  return 0;
}

// A zeroed device buffer of the sim's; `what` names it in the error.
template <class T>
static int device_zeros(T** p, size_t bytes, const char* what) {
  hipError_t e = hipMalloc((void**)p, bytes);
  if (e == hipSuccess) e = hipMemset(*p, 0, bytes);
  if (e != hipSuccess) return fail(std::string("hipMalloc ") + what + ": " + hipGetErrorString(e));
  return 0;
}

extern "C" {

const char* mjx_last_error(void) { return g_err.c_str(); }
int mjx_abi_version(void) { return MJX_ABI_VERSION; }
size_t mjx_model_desc_size(void) { return sizeof(mjxModelDesc); }

int mjx_model_create(const mjxModelDesc* desc, int device, mjxModel** out) {
  if (!desc || !out) return fail("null argument");
  auto m = std::make_unique<mjxModel_>();
  {
    // every check of the descriptor, and all host derivation (model_tables.h)
    const std::string err = mjx::build_model_tables(*desc, m->t);
    if (!err.empty()) return fail(err);
  }
  HIPCHK(hipSetDevice(device));
  m->device = device;
  // (a host that leaves the appended sensor_cutoff null has no cutoffs)
  mjxModelDesc with_cutoff = *desc;
  const std::vector<double> no_cutoff(desc->nsensor > 0 ? desc->nsensor : 1, 0.0);
  if (!with_cutoff.sensor_cutoff) with_cutoff.sensor_cutoff = no_cutoff.data();
  desc = &with_cutoff;
  const mjx::ModelTables& t = m->t;
  mjx::DModel& dm = m->dm;
  // the descriptor's arrays (fields.h counts them over `d`; the pair lists are uploaded whole,
  // regular and terrain pairs)
  // `d` as fields.h counts over it: the dims and the number of equalities (DModel::neq)
  struct FieldDims : mjx::Dims { int neq; } d{t.d, t.neq};
  d.npair = t.d.npair_all;
#define X_INT(name, cnt, w)                                                              \
  {                                                                                      \
    const size_t n_ = (size_t)(cnt) * (w);                                               \
    if (upload(m.get(), std::vector<int32_t>(desc->name, desc->name + n_), dm.name)) return -1; \
    m->int_dims[#name] = {(int64_t)(cnt), (int64_t)(w)};                                 \
  }
#define X_FLT(name, cnt, w)                                                              \
  {                                                                                      \
    const size_t n_ = (size_t)(cnt) * (w);                                               \
    std::vector<float> h_(desc->name, desc->name + n_);                                  \
    if (upload(m.get(), h_, dm.name)) return -1;                                         \
    dm.name##_ws = 0;                                                                    \
    m->host_float[#name] = std::move(h_);                                                \
    m->float_dims[#name] = {(int64_t)(cnt), (int64_t)(w)};                               \
  }
  MJX_MODEL_INT_FIELDS(X_INT)
  MJX_MODEL_FLOAT_FIELDS(X_FLT)
#undef X_INT
#undef X_FLT
  if (upload(m.get(), std::vector<uint64_t>(desc->dof_bodymask, desc->dof_bodymask + d.nv), dm.dof_bodymask))
    return -1;
  // the derived tables
  dm.nmaskword = t.nmaskword;
  dm.neq = t.neq;
  dm.max_condim = t.max_condim;
  dm.ncsens = t.ncsens;
  const size_t nmask = (size_t)desc->nmaskword * d.nsensor;
  if (upload(m.get(), t.dof_ancmask, dm.dof_ancmask) || upload(m.get(), t.body_submask, dm.body_submask) ||
      upload(m.get(), t.body_dofmask, dm.body_dofmask) ||
      upload(m.get(), t.body_rec, dm.body_rec, mjx::kBodyRec) ||
      upload(m.get(), t.dof_rec, dm.dof_rec, mjx::kDofRec) ||
      upload(m.get(), t.act_rec, dm.act_rec, mjx::kActRec) ||
      upload(m.get(), t.geom_lds, dm.geom_lds) || upload(m.get(), t.lds_geom, dm.lds_geom) ||
      upload(m.get(), t.st_geom, dm.st_geom) || upload(m.get(), t.st_pairadr, dm.st_pairadr) ||
      upload(m.get(), t.st_partner, dm.st_partner) || upload(m.get(), t.st_aabb, dm.st_aabb, 6) ||
      upload(m.get(), t.st_chunk_aabb, dm.st_chunk_aabb) ||
      // (without records phase A reads a pair's geoms one by one)
      (!t.pair_rec.empty() && upload(m.get(), t.pair_rec, dm.pair_rec)) ||
      upload(m.get(), std::vector<uint32_t>(desc->sensor_geommask1, desc->sensor_geommask1 + nmask), dm.sensor_geommask1) ||
      upload(m.get(), std::vector<uint32_t>(desc->sensor_geommask2, desc->sensor_geommask2 + nmask), dm.sensor_geommask2) ||
      upload(m.get(), t.cs_sensor, dm.cs_sensor) || upload(m.get(), t.geom_csmask1, dm.geom_csmask1) ||
      upload(m.get(), t.geom_csmask2, dm.geom_csmask2))
    return -1;
  // (no extended sensor: sensor_ext.hip is never launched)
  if (!t.sensor_ext.empty() && upload(m.get(), t.sensor_ext, m->ext.rec)) return -1;
  m->ext.n = (int)t.sensor_ext.size();
  *out = m.release();
  return 0;
}

int mjx_model_destroy(mjxModel* m) {
  if (m) delete m;
  return 0;
}

int mjx_sim_create(const mjxModel* model, int nworld, int nconmax, int njmax, mjxSim** out) {
  return mjx_sim_create_ex(model, nworld, nconmax, njmax, nconmax, njmax, out);
}

int mjx_sim_create_ex(const mjxModel* model, int nworld, int nconmax, int njmax,
                      int nconmax_max, int njmax_max, mjxSim** out) {
  if (!model || !out) return fail("null argument");
  if (nworld <= 0) return fail("nworld must be positive");
  if (nconmax <= 0 || nconmax > mjx::kWave)
    return fail("nconmax (contacts held per world) must be in [1, 64]");
  if (njmax <= 0) return fail("njmax must be positive");
  if (njmax < 2 * model->t.neq)
    return fail("njmax below the model's equality rows (two per equality constraint)");
  if (model->t.max_condim > 3 && njmax_max < 2 * model->t.neq + 2 * (model->t.max_condim - 1))
    return fail("njmax_max below one contact of the model's largest condim (2 (condim - 1) rows "
                "behind the equality rows)");
  if (nconmax_max < nconmax || nconmax_max > mjx::kMaxContacts || njmax_max < njmax)
    return fail("max capacity: nconmax <= nconmax_max <= 512 and njmax <= njmax_max");
  if (nconmax_max > mjx::kWave && nconmax_max > njmax_max)
    return fail("a max capacity past 64 contacts needs njmax_max >= nconmax_max (the contact sort's "
                "scratch is the row block)");
  HIPCHK(hipSetDevice(model->device));
  auto owner = std::make_unique<mjxSim_>();
  mjxSim_* s = owner.get();
  s->model = model;
  s->nworld = nworld;
  s->dm = model->dm;
  mjx::Dims dims = model->t.d;
  dims.nconmax = nconmax;
  dims.njmax = njmax;
  if (make_capacity(dims, model->t.dof_parentid, model->t.neq, model->t.max_condim,
                    model->t.o.cone, "per-world LDS footprint exceeds 160 KiB; lower njmax/nconmax", s->fast))
    return -1;
  // An elliptic model runs without Newton row classes: a class launch copies the pack's row
  // slots region by region into its smaller carve, and the grouping words (carve.h make_lds)
  // are not among them.  Every world then takes the full-capacity carve: the range chain, phase
  // B, the masked forward and the re-solve, all of which hold the cone solver.
  s->nrowclass = model->t.o.cone != 0 ? 0 : mjx::choose_row_classes(s->fast.d, s->fast.spec, s->row_cap);
  // batch splits (launch_step): large batches of models without row classes run as
  // concurrent halves.  MJX355_SPLIT=<n> overrides (diagnostic; 1 = one launch set per phase),
  // also for models with row classes (each split then forks its own class streams).
  s->side.nsplit = nworld >= mjx::kSplitMinWorlds && s->nrowclass == 0 ? 2 : 1;
  if (const char* ev = getenv("MJX355_SPLIT")) s->side.nsplit = std::max(1, std::min(atoi(ev), mjx::kMaxSplit));
  // The overflow re-solve forks its chain from the stream that ran phase A.  With batch
  // splits that is a split stream, and a second-level fork from a captured side stream
  // crashes hipStreamEndCapture under the HIP runtime torch bundles:
  // split batches without row classes run the chain in line on their split stream instead
  // (launch_step); split batches with row classes (a diagnostic topology) keep the fast
  // carve as their max capacity (overflow drops, counted).
  s->has_big = (nconmax_max > nconmax || njmax_max > njmax) &&
               (s->side.nsplit == 1 || s->nrowclass == 0);
  s->con_stride = s->has_big ? nconmax_max : nconmax;
  if (s->has_big) {
    dims.nconmax = nconmax_max;
    dims.njmax = njmax_max;
    if (make_capacity(dims, model->t.dof_parentid, model->t.neq, model->t.max_condim,
                      model->t.o.cone, "max-capacity LDS footprint exceeds 160 KiB; lower njmax_max/nconmax_max", s->big))
      return -1;
    // re-solve list capacity per split and substep parity: every world may be listed
    s->ovf_cap = nworld;
  }
  for (int k = 0; k < mjx::kRowClasses; k++) {
    mjx::Dims ds = s->fast.d;
    ds.njmax = k < s->nrowclass ? s->row_cap[k] : s->fast.d.njmax;
    s->lds_class[k] = mjx::make_lds(ds, 1, false, 2, model->t.o.cone);
  }
  {
    hipError_t e = hipSuccess;
    if (s->side.nsplit > 1) {
      e = hipEventCreateWithFlags(&s->side.split_fork, hipEventDisableTiming);
      for (int p = 1; p < s->side.nsplit && e == hipSuccess; p++) {
        e = hipStreamCreateWithFlags(&s->side.split[p], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->side.split_join[p], hipEventDisableTiming);
      }
    }
    // default priority: measured, high-priority side streams let the few heavy worlds hold
    // LDS that the bulk of small-class worlds needs (Newton span 214 -> 281 us, G1 4096)
    for (int p = 0; p < s->side.nsplit && s->nrowclass > 0 && e == hipSuccess; p++) {
      e = hipEventCreateWithFlags(&s->side.fork[p], hipEventDisableTiming);
      for (int k = 0; k < s->nrowclass && e == hipSuccess; k++) {
        e = hipStreamCreateWithFlags(&s->side.stream[p][k], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->side.join[p][k], hipEventDisableTiming);
      }
    }
    for (int p = 0; p < s->side.nsplit && s->has_big && e == hipSuccess; p++) {
      e = hipStreamCreateWithFlags(&s->side.ovf[p], hipStreamNonBlocking);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&s->side.ovf_fork[p], hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&s->side.ovf_join[p], hipEventDisableTiming);
    }
    if (e != hipSuccess) return fail(std::string("side streams: ") + hipGetErrorString(e));
  }
  // the contact output arrays hold the max capacity's contacts
  mjx::Dims d = s->fast.d;
  d.nconmax = s->con_stride;
  // data arena: one allocation, 256-B aligned sub-buffers
  size_t off = 0;
  std::vector<std::pair<std::string, size_t>> offs;
  auto reserve = [&](const std::string& name, size_t bytes) {
    offs.push_back({name, off});
    off += (bytes + 255) & ~(size_t)255;
  };
#define X_FLT(name, cnt, w) reserve(#name, sizeof(float) * (size_t)nworld * (cnt) * (w));
#define X_INT(name, cnt, w) reserve(#name, sizeof(int32_t) * (size_t)nworld * (cnt) * (w));
  MJX_DATA_FLOAT_FIELDS(X_FLT)
  MJX_DATA_INT_FIELDS(X_INT)
#undef X_FLT
#undef X_INT
  reserve("__stats", sizeof(int32_t) * 8);
  reserve("__wstats", sizeof(int32_t) * 8 * (size_t)nworld);
  reserve("__evtotal", sizeof(int32_t) * 4);
  reserve("__prof", sizeof(unsigned long long) * 48);
  reserve("__wtrace", sizeof(unsigned long long) * 8 * (size_t)nworld);
  reserve("contact_torque", sizeof(float) * (size_t)nworld * d.nconmax * 3);
  if (device_zeros(&s->fast.gscr, sizeof(float) * (size_t)nworld * s->fast.gstride, "scratch") ||
      device_zeros(&s->wl, sizeof(int) * ((size_t)nworld + 2 * (mjx::kRowClasses + 1) * mjx::kMaxSplit),
                   "work lists"))
    return -1;
  if (s->has_big &&
      (device_zeros(&s->big.gscr, sizeof(float) * (size_t)nworld * s->big.gstride, "re-solve buffers") ||
       device_zeros(&s->ovf, sizeof(int) * ((size_t)mjx::kMaxSplit * 2 * (s->ovf_cap + 2) + nworld),
                    "re-solve buffers") ||
       device_zeros(&s->big.dparams, sizeof(mjx::Params), "re-solve buffers")))
    return -1;
  if (device_zeros(&s->arena, off, "data")) return -1;
  size_t k = 0;
  char* base = (char*)s->arena;
  // a field whose count is the literal 1 (fields.h) is a per-world scalar; every other keeps
  // its count axis even when the model makes it 1 (qpos of a one-dof model is [nworld, 1])
#define X_FLT(name, cnt, w)                                                                  \
  s->dd.name = (float*)(base + offs[k++].second);                                            \
  s->fields[#name] = FieldInfo{s->dd.name, true, (int64_t)(cnt), (int64_t)(w), true, false,  \
                               std::string(#cnt) == "1"};                                    \
  s->names.push_back(#name);
#define X_INT(name, cnt, w)                                                                    \
  s->dd.name = (int32_t*)(base + offs[k++].second);                                            \
  s->fields[#name] = FieldInfo{s->dd.name, false, (int64_t)(cnt), (int64_t)(w), true, false,  \
                               std::string(#cnt) == "1"};                                      \
  s->names.push_back(#name);
  MJX_DATA_FLOAT_FIELDS(X_FLT)
  MJX_DATA_INT_FIELDS(X_INT)
#undef X_FLT
#undef X_INT
  // an unused contact slot holds geoms (-1, -1), as the outputs leave every slot past ncon
  // (a slot never written must read the same as one cleared: fused and single steps write
  // outputs on different substeps)
  HIPCHK(hipMemset(s->dd.contact_geom, 0xff, sizeof(int32_t) * (size_t)nworld * d.nconmax * 2));
  s->dd.stats = (int32_t*)(base + offs[k++].second);
  s->dd.wstats = (int32_t*)(base + offs[k++].second);
  // per-world engine counters [nworld, 8] (phase C, last substep): [0] contacts found,
  // [1] rows, [2] contact-overflow / [3] row-overflow / [4] unsupported-pair events
  // (cumulative), [5] Newton iterations -- a zero-copy view for device-side logging
  s->fields["engine_counters"] = FieldInfo{s->dd.wstats, false, 8, 1, true, false};
  s->names.push_back("engine_counters");
  // [1, 4]: contact-overflow / row-overflow / unsupported-pair events summed over worlds
  s->dd.evtotal = (int32_t*)(base + offs[k++].second);
  s->fields["engine_events"] = FieldInfo{s->dd.evtotal, false, 4, 1, false, false};
  s->names.push_back("engine_events");
  s->dd.prof = (unsigned long long*)(base + offs[k++].second);
  // per-world phase start/end timestamps (s_memrealtime, 100 MHz; diagnostic MJX_STAMPS
  // build): [A0 A1 B0 B1 C0 C1 - -] as int32 pairs
  s->dd.wtrace = (unsigned long long*)(base + offs[k++].second);
  s->fields["world_trace"] = FieldInfo{s->dd.wtrace, false, 16, 1, true, false};
  s->names.push_back("world_trace");
  // torsional / rolling contact torque in the contact frame, beside contact_force (the pointer
  // travels in the sim's model copy: engine.h DModel)
  s->dm.contact_torque = (float*)(base + offs[k++].second);
  s->fields["contact_torque"] = FieldInfo{s->dm.contact_torque, true, (int64_t)d.nconmax, 3, true, false, false};
  s->names.push_back("contact_torque");
  // model fields visible as "model.<name>"
  for (auto& kv : model->float_dims) {
    FieldInfo fi{nullptr, true, kv.second.first, kv.second.second, false, true};
    s->fields["model." + kv.first] = fi;
    s->names.push_back("model." + kv.first);
  }
  for (auto& kv : model->int_dims) {
    FieldInfo fi{nullptr, false, kv.second.first, kv.second.second, false, true};
    s->fields["model." + kv.first] = fi;
    s->names.push_back("model." + kv.first);
  }
  if (device_zeros(&s->fast.dparams, sizeof(mjx::Params), "params") || sync_params(s, nullptr)) return -1;
  hipError_t e = mjx::prepare_step(s->host);
  if (e == hipSuccess && s->has_big) e = mjx::prepare_step(s->host_big);
  s->side.range_chain = s->nrowclass == 0 && mjx::range_chain_default(s->host, nworld, s->side.nsplit);
  if (e != hipSuccess) return fail(std::string("prepare: ") + hipGetErrorString(e));
  // heightfield geom frames are static: write them once for every world
  const mjx::ModelTables& t = model->t;
  for (size_t k = 0; k < t.static_geoms.size(); k++) {
    const int g = t.static_geoms[k];
    std::vector<float> px((size_t)nworld * 3), pm((size_t)nworld * 9);
    for (int w = 0; w < nworld; w++) {
      for (int i = 0; i < 3; i++) px[(size_t)w * 3 + i] = t.static_xpos[3 * k + i];
      for (int i = 0; i < 9; i++) pm[(size_t)w * 9 + i] = t.static_xmat[9 * k + i];
    }
    e = hipMemcpy2D(s->dd.geom_xpos + 3 * g, sizeof(float) * 3 * d.ngeom, px.data(),
                    sizeof(float) * 3, sizeof(float) * 3, nworld, hipMemcpyHostToDevice);
    if (e == hipSuccess)
      e = hipMemcpy2D(s->dd.geom_xmat + 9 * g, sizeof(float) * 9 * d.ngeom, pm.data(),
                      sizeof(float) * 9, sizeof(float) * 9, nworld, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(std::string("hfield frames: ") + hipGetErrorString(e));
  }
  // initial state: mj_resetData
  if (mjx::launch_reset(d, s->dm, s->dd, nullptr, nworld, s->con_stride, nullptr) != hipSuccess)
    return fail("reset launch failed");
  e = hipDeviceSynchronize();
  if (e != hipSuccess) return fail(std::string("sync: ") + hipGetErrorString(e));
  *out = owner.release();
  return 0;
}

int mjx_sim_destroy(mjxSim* s) {
  if (s) delete s;
  return 0;
}

int mjx_step(mjxSim* s, int nsubstep, void* stream) {
  if (!s) return fail("null sim");
  if (nsubstep < 1) return fail("nsubstep must be >= 1");
  hipError_t e = mjx::launch_step(s->host, s->fast.dparams, s->nworld, nsubstep, 1, nullptr,
                                  (hipStream_t)stream, &s->side, s->has_big ? &s->host_big : nullptr,
                                  s->big.dparams, &s->model->ext);
  if (e != hipSuccess) return fail(std::string("step launch: ") + hipGetErrorString(e));
  return 0;
}

int mjx_forward(mjxSim* s, void* stream) { return mjx_forward_masked(s, nullptr, stream); }

int mjx_forward_masked(mjxSim* s, const uint8_t* mask, void* stream) {
  if (!s) return fail("null sim");
  hipError_t e = mjx::launch_step(s->host, s->fast.dparams, s->nworld, 1, 0, mask,
                                  (hipStream_t)stream, &s->side, s->has_big ? &s->host_big : nullptr,
                                  s->big.dparams, &s->model->ext);
  if (e != hipSuccess) return fail(std::string("forward launch: ") + hipGetErrorString(e));
  return 0;
}

int mjx_sim_track_air_time(mjxSim* s, int n, const int32_t* found_adr, float* cur_air,
                           float* last_air, float* cur_contact, float* last_contact,
                           float* last_time, void* stream) {
  if (!s) return fail("null sim");
  if (n < 0 || n > mjx::kMaxAirSlots) return fail("air-time tracking: 0 <= n <= 8 slots");
  if (n > 0 && (!found_adr || !cur_air || !last_air || !cur_contact || !last_contact || !last_time))
    return fail("air-time tracking: null buffer");
  for (int i = 0; i < n; i++)
    if (found_adr[i] < 0 || found_adr[i] >= s->fast.d.nsensordata)
      return fail("air-time tracking: found address outside sensordata");
  s->nair = n;
  for (int i = 0; i < mjx::kMaxAirSlots; i++) s->air_found[i] = i < n ? found_adr[i] : 0;
  float* b[5] = {cur_air, last_air, cur_contact, last_contact, last_time};
  for (int i = 0; i < 5; i++) s->air_buf[i] = n > 0 ? b[i] : nullptr;
  return sync_params(s, stream);
}

size_t mjx_actuator_desc_size(void) { return sizeof(mjxActuatorDesc); }

// Unbind the actuator networks (host side; the caller uploads the parameters).  The stream is
// drained first: a launch in flight may still read the weights.
static int drop_actuator_nets(mjxSim_* s, void* stream) {
  if (s->netw) {
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(hipDeviceSynchronize());
    (void)hipFree(s->netw);
    s->netw = nullptr;
  }
  s->net = mjx::NetParams{};
  for (int u = 0; u < mjx::kWave; u++) s->net.net_of[u] = mjx::kNoNet;
  return 0;
}

int mjx_sim_set_actuators(mjxSim* s, const mjxActuatorDesc* a, void* stream) {
  if (!a) {  // off: phase A takes every actuator's ctrl as it is
    if (!s) return fail("null sim");
    if (drop_actuator_nets(s, stream)) return -1;
    s->act_on = false;
    s->act = mjx::ActParams{};
    return sync_params(s, stream);
  }
  const char* const who = "mjx_sim_set_actuators: ";
  // the descriptor's own consistency first (it needs no sim), then its fit to the sim
  if (a->nworld < 1) return fail(std::string(who) + "nworld < 1");
  if (a->nu < 1 || a->nu > mjx::kWave) return fail(std::string(who) + "1 <= nu <= 64");
  if (a->ring_len < 0 || a->ring_len > mjx::kMaxActLag)
    return fail(std::string(who) + "0 <= ring_len <= 32");
  if (!a->kind || !a->min_lag || !a->max_lag || !a->group)
    return fail(std::string(who) + "null kind / min_lag / max_lag / group table");
  bool any = false, pd = false, dc = false, delayed = false;
  for (int u = 0; u < a->nu; u++) {
    const int k = a->kind[u];
    if (k != mjx::kActBuiltin && k != mjx::kActDelayed && k != mjx::kActIdealPd &&
        k != mjx::kActDcMotor)
      return fail(std::string(who) +
                  "kind must be 0 (builtin), 1 (delayed builtin), 2 (ideal PD) or 3 (DC motor)");
    if (a->min_lag[u] > a->max_lag[u]) return fail(std::string(who) + "min_lag > max_lag");
    if (a->max_lag[u] > a->ring_len) return fail(std::string(who) + "max_lag exceeds ring_len");
    if (k == mjx::kActBuiltin && a->max_lag[u] != 0)
      return fail(std::string(who) + "a builtin actuator cannot be delayed");
    any |= k != mjx::kActBuiltin;
    dc |= k == mjx::kActDcMotor;
    pd |= k == mjx::kActIdealPd || k == mjx::kActDcMotor;
    delayed |= a->max_lag[u] > 0;
  }
  if (!any) return fail(std::string(who) + "no explicit actuator (pass a null descriptor to turn them off)");
  if (!a->position_target) return fail(std::string(who) + "null position_target buffer");
  if (pd && (!a->kp || !a->kd || !a->effort_limit || !a->velocity_target || !a->effort_target))
    return fail(std::string(who) + "null gain / limit / target buffer");
  if (dc && (!a->saturation_effort || !a->velocity_limit || !a->corner_velocity))
    return fail(std::string(who) + "null DC motor buffer");
  if (delayed && (!a->ring || !a->lag || !a->pushes || !a->draws))
    return fail(std::string(who) + "null delay buffer");
  if (!s) return fail(std::string(who) + "null sim");
  if (a->nworld != s->nworld) return fail(std::string(who) + "nworld differs from the sim's");
  if (a->nu != s->fast.d.nu) return fail(std::string(who) + "nu differs from the model's");
  mjx::ActParams p{};
  for (int u = 0; u < a->nu; u++) {
    p.kind[u] = a->kind[u]; p.min_lag[u] = a->min_lag[u]; p.max_lag[u] = a->max_lag[u];
    p.group[u] = a->group[u];
  }
  p.ring_len = delayed ? a->ring_len : 0;
  p.seed = a->seed;
  p.kp = a->kp; p.kd = a->kd; p.flim = a->effort_limit;
  p.sat = a->saturation_effort; p.vlim = a->velocity_limit; p.vcorner = a->corner_velocity;
  p.pt = a->position_target; p.vt = a->velocity_target; p.ft = a->effort_target;
  p.ring = a->ring; p.lag = a->lag; p.pushes = a->pushes; p.draws = a->draws;
  p.hold = a->hold;
  if (drop_actuator_nets(s, stream)) return -1;  // a new binding has no networks yet
  s->act = p;
  s->act_on = true;
  return sync_params(s, stream);
}

size_t mjx_actuator_net_desc_size(void) { return sizeof(mjxActuatorNetDesc); }

int mjx_sim_set_actuator_nets(mjxSim* s, const mjxActuatorNetDesc* a, void* stream) {
  const std::string who = "mjx_sim_set_actuator_nets: ";
  if (!a) {  // off: the bound actuators keep their kinds, the learned ones fall back to kp = kd = 0
    if (!s) return fail(who + "null sim");
    if (drop_actuator_nets(s, stream)) return -1;
    return sync_params(s, stream);
  }
  static_assert(MJX_MAX_ACT_NETS == mjx::kMaxNets && MJX_MAX_NET_LAYERS == mjx::kMaxNetLayers, "");
  // the descriptor's own consistency first (it needs no sim), then its fit to the sim
  if (a->nworld < 1) return fail(who + "nworld < 1");
  if (a->nu < 1 || a->nu > mjx::kWave) return fail(who + "1 <= nu <= 64");
  if (a->nnet < 1 || a->nnet > mjx::kMaxNets) return fail(who + "1 <= nnet <= 4");
  int hmax = 0;
  for (int k = 0; k < a->nnet; k++) {
    const mjxActuatorNet& n = a->nets[k];
    if (n.nlayer < 1 || n.nlayer > mjx::kMaxNetLayers) return fail(who + "1 <= nlayer <= 4");
    if (n.history < 1 || n.history > mjx::kMaxNetHist) return fail(who + "1 <= history <= 8");
    if (n.input_order != 0 && n.input_order != 1)
      return fail(who + "input_order must be 0 (pos_vel) or 1 (vel_pos)");
    for (int l = 0; l <= n.nlayer; l++)
      if (n.width[l] < 1 || n.width[l] > mjx::kMaxNetWidth) return fail(who + "1 <= width <= 32");
    if (n.width[0] != 2 * n.history) return fail(who + "the input width must be 2 * history");
    if (n.width[n.nlayer] != 1) return fail(who + "the output width must be 1");
    for (int l = 0; l < n.nlayer; l++) {
      if (n.activation[l] < mjx::kNetNone || n.activation[l] > mjx::kNetElu)
        return fail(who + "activation must be 0 (none), 1 (relu), 2 (softsign), 3 (tanh) or 4 (elu)");
      if (!n.weight[l] || !n.bias[l]) return fail(who + "null weight / bias");
    }
    if (n.activation[n.nlayer - 1] != mjx::kNetNone)
      return fail(who + "no activation after the last layer");
    hmax = n.history - 1 > hmax ? n.history - 1 : hmax;
  }
  if (a->hist_len != hmax) return fail(who + "hist_len must be the largest history - 1");
  if (!a->net) return fail(who + "null net table");
  bool any = false;
  for (int u = 0; u < a->nu; u++) {
    if (a->net[u] != mjx::kNoNet && a->net[u] >= a->nnet) return fail(who + "net[u] out of range");
    any |= a->net[u] != mjx::kNoNet;
  }
  if (!any) return fail(who + "no actuator has a network (pass a null descriptor to unbind)");
  if (hmax > 0 && (!a->history || !a->staging || !a->pushes))
    return fail(who + "null history / staging / pushes buffer");
  if (!s) return fail(who + "null sim");
  if (a->nworld != s->nworld) return fail(who + "nworld differs from the sim's");
  if (a->nu != s->fast.d.nu) return fail(who + "nu differs from the model's");
  if (!s->act_on) return fail(who + "no explicit actuators bound (mjx_sim_set_actuators comes first)");
  for (int u = 0; u < a->nu; u++)
    if (a->net[u] != mjx::kNoNet && s->act.kind[u] != mjx::kActDcMotor)
      return fail(who + "net[u] on an actuator whose kind is not 3 (DC motor)");
  // pack: per layer [32][32] W (row = output, zero padded) then 32 biases
  std::vector<float> w((size_t)a->nnet * mjx::kNetStride, 0.f);
  for (int k = 0; k < a->nnet; k++) {
    const mjxActuatorNet& n = a->nets[k];
    for (int l = 0; l < n.nlayer; l++) {
      float* dst = w.data() + (size_t)k * mjx::kNetStride + (size_t)l * mjx::kNetLayerStride;
      const int nin = n.width[l], nout = n.width[l + 1];
      for (int o = 0; o < nout; o++) {
        for (int i = 0; i < nin; i++) dst[o * mjx::kMaxNetWidth + i] = n.weight[l][(size_t)o * nin + i];
        dst[mjx::kMaxNetWidth * mjx::kMaxNetWidth + o] = n.bias[l][o];
      }
    }
  }
  if (drop_actuator_nets(s, stream)) return -1;
  // (from here the old networks are gone: a failure uploads the cleared parameters, so the
  // device never keeps the freed pointer)
  hipError_t e = hipMalloc((void**)&s->netw, w.size() * sizeof(float));
  if (e == hipSuccess)
    e = hipMemcpy(s->netw, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (s->netw) (void)hipFree(s->netw);
    s->netw = nullptr;
    (void)sync_params(s, stream);
    return fail(who + "weight upload: " + hipGetErrorString(e));
  }
  mjx::NetParams& p = s->net;
  p.nnet = a->nnet;
  p.hist_len = hmax;
  p.netw = s->netw;
  p.hist = a->history; p.stage = a->staging; p.hpush = a->pushes;
  for (int k = 0; k < a->nnet; k++) {
    const mjxActuatorNet& n = a->nets[k];
    mjx::NetMeta& M = p.net[k];
    M = mjx::NetMeta{};
    M.nlayer = (uint8_t)n.nlayer; M.hist = (uint8_t)n.history; M.vel_first = (uint8_t)n.input_order;
    for (int l = 0; l < n.nlayer; l++) {
      M.nin[l] = (uint8_t)n.width[l]; M.nout[l] = (uint8_t)n.width[l + 1];
      M.act[l] = (uint8_t)n.activation[l];
    }
    M.pos_scale = n.pos_scale; M.vel_scale = n.vel_scale; M.torque_scale = n.torque_scale;
  }
  for (int u = 0; u < mjx::kWave; u++) {
    p.net_of[u] = u < a->nu ? a->net[u] : (uint8_t)mjx::kNoNet;
    p.net_hist[u] = p.net_of[u] != mjx::kNoNet ? (uint8_t)a->nets[p.net_of[u]].history : 0;
  }
  return sync_params(s, stream);
}

int mjx_reset(mjxSim* s, const uint8_t* mask, void* stream) {
  if (!s) return fail("null sim");
  hipError_t e = mjx::launch_reset(s->fast.d, s->dm, s->dd, mask, s->nworld, s->con_stride, (hipStream_t)stream);
  if (e != hipSuccess) return fail(std::string("reset launch: ") + hipGetErrorString(e));
  return 0;
}

static void dl_deleter(DLManagedTensor* t) {
  if (!t) return;
  delete[] t->dl_tensor.shape;
  delete t;
}

static const void* model_field_ptr(const mjxSim_* s, const std::string& name, int* ws) {
  *ws = 0;
#define X_FLT(n, cnt, w) if (name == #n) { *ws = s->dm.n##_ws; return s->dm.n; }
#define X_INT(n, cnt, w) if (name == #n) { return s->dm.n; }
  MJX_MODEL_FLOAT_FIELDS(X_FLT)
  MJX_MODEL_INT_FIELDS(X_INT)
#undef X_FLT
#undef X_INT
  return nullptr;
}

int mjx_field(mjxSim* s, const char* cname, DLManagedTensor** out) {
  if (!s || !cname || !out) return fail("null argument");
  std::string name(cname);
  auto it = s->fields.find(name);
  if (it == s->fields.end()) return fail("unknown field '" + name + "'");
  const FieldInfo& fi = it->second;
  void* ptr = fi.ptr;
  int64_t lead = fi.per_world ? s->nworld : 1;
  if (fi.model) {
    int ws = 0;
    ptr = const_cast<void*>(model_field_ptr(s, name.substr(6), &ws));
    lead = ws > 0 ? s->nworld : 1;
  }
  auto* t = new DLManagedTensor();
  std::vector<int64_t> shape;
  shape.push_back(lead);
  if (!fi.scalar) shape.push_back(fi.count);
  if (fi.width > 1) shape.push_back(fi.width);
  t->dl_tensor.data = ptr;
  t->dl_tensor.device = DLDevice{kDLROCM, s->model->device};
  t->dl_tensor.ndim = (int32_t)shape.size();
  t->dl_tensor.dtype = fi.is_float ? DLDataType{2, 32, 1} : DLDataType{0, 32, 1};
  t->dl_tensor.shape = new int64_t[shape.size()];
  for (size_t i = 0; i < shape.size(); i++) t->dl_tensor.shape[i] = shape[i];
  t->dl_tensor.strides = nullptr;  // compact row-major
  t->dl_tensor.byte_offset = 0;
  t->manager_ctx = nullptr;
  t->deleter = dl_deleter;
  *out = t;
  return 0;
}

int mjx_field_count(const mjxSim* s) { return s ? (int)s->names.size() : 0; }
const char* mjx_field_name(const mjxSim* s, int i) {
  if (!s || i < 0 || i >= (int)s->names.size()) return nullptr;
  return s->names[i].c_str();
}

int mjx_field_is_expanded(const mjxSim* s, const char* cname) {
  if (!s || !cname) return 0;
  int ws = 0;
  model_field_ptr(s, std::string(cname), &ws);
  return ws > 0;
}

int mjx_expand_field(mjxSim* s, const char* cname, void* stream) {
  if (!s || !cname) return fail("null argument");
  std::string name(cname);
  auto hit = s->model->host_float.find(name);
  if (hit == s->model->host_float.end())
    return fail("field '" + name + "' is not an expandable float model field");
  const std::vector<float>& h = hit->second;
  size_t per = h.size();
  // tile the CURRENT values (default model values) to every world
  int ws = 0;
  const float* cur = (const float*)model_field_ptr(s, name, &ws);
  if (ws > 0) return fail("field '" + name + "' already expanded");
  float* buf = nullptr;
  size_t bytes = sizeof(float) * (per > 0 ? per : 1) * (size_t)s->nworld;
  HIPCHK(hipMalloc((void**)&buf, bytes));
  s->expanded_allocs.push_back(buf);
  // world 0 from the model, then doubling copies of the filled prefix: ceil(log2 N) + 1
  // copies instead of one per world (8,192 copy dispatches for Go1 at sim creation)
  if (s->nworld > 0)
    HIPCHK(hipMemcpyAsync(buf, cur, sizeof(float) * per, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  for (size_t done = 1; done < (size_t)s->nworld;) {
    const size_t n = std::min(done, (size_t)s->nworld - done);
    HIPCHK(hipMemcpyAsync(buf + done * per, buf, sizeof(float) * per * n, hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
    done += n;
  }
#define X_FLT(n, cnt, w) if (name == #n) { s->dm.n = buf; s->dm.n##_ws = (int)per; }
  MJX_MODEL_FLOAT_FIELDS(X_FLT)
#undef X_FLT
  return sync_params(s, stream);
}

int mjx_sim_profile(mjxSim* s, uint64_t* out, void* stream) {
  if (!s || !out) return fail("null argument");
  HIPCHK(hipMemcpyAsync(out, s->dd.prof, sizeof(uint64_t) * 48, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

int mjx_sim_spec(const mjxSim* s) { return s ? s->fast.spec : -1; }

int mjx_spec_register(const char* path) {
  if (!path) return fail("null path");
  void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!h) return fail(std::string("dlopen: ") + dlerror());
  using AbiFn = int (*)(void);
  using DimsFn = void (*)(mjx::Dims*);
  using TreeFn = int (*)(int*, int);
  using KernFn = mjx::StepFnPtr (*)(int);
  auto abi = reinterpret_cast<AbiFn>(dlsym(h, "mjx_jit_abi"));
  auto dims = reinterpret_cast<DimsFn>(dlsym(h, "mjx_jit_dims"));
  auto tree = reinterpret_cast<TreeFn>(dlsym(h, "mjx_jit_tree"));
  auto kern = reinterpret_cast<KernFn>(dlsym(h, "mjx_jit_kernel"));
  if (!abi || !dims || !tree || !kern) return fail(std::string(path) + ": not a jit.hip library");
  if (abi() != (int)sizeof(mjx::Dims)) return fail(std::string(path) + ": Dims layout mismatch (stale build)");
  // the kernels read Params / Lds / DData through this library's layout: the JIT library must
  // come from the same kernel headers (csrc/Makefile MJX_HDR_HASH), else a stale cache entry or
  // a header edited after the last engine build would fault the device instead of failing here
  using HdrFn = unsigned long long (*)(void);
  auto hdr = reinterpret_cast<HdrFn>(dlsym(h, "mjx_jit_hdr"));
#ifdef MJX_HDR_HASH
  if (!hdr || hdr() != (unsigned long long)MJX_HDR_HASH)
    return fail(std::string(path) + ": built from other kernel headers than libmjx355.so (rebuild one of them)");
#else
  if (!hdr) return fail(std::string(path) + ": not a jit.hip library of this engine");
#endif
  mjx::Dims d{};
  dims(&d);
  int par[64];
  const int n = tree(par, 64);
  if (n < 0 || n > 64) return fail("bad dof tree in the jit library");
  return mjx::register_spec(d, par, n, kern);  // the library stays loaded for the process
}

int mjx_sim_mass_matrix(mjxSim* s, int big, float* out, void* stream) {
  if (!s || !out) return fail("null argument");
  if (big && !s->has_big) return fail("the sim has no max-capacity scratch");
  const int nvp = (s->fast.d.nv + 3) & ~3;
  const size_t n = (size_t)mjx::ltr_size(nvp);
  const Capacity& c = big ? s->big : s->fast;
  const float* src = c.gscr + c.lds[1].M;
  const size_t pitch = sizeof(float) * (size_t)c.gstride;
  HIPCHK(hipMemcpy2DAsync(out, sizeof(float) * n, src, pitch, sizeof(float) * n, s->nworld,
                          hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int mjx_sim_info(const mjxSim* s, int32_t* out) {
  if (!s || !out) return fail("null argument");
  const mjx::Dims& top = s->has_big ? s->big.d : s->fast.d;
  const int32_t v[8] = {s->fast.d.nconmax, s->fast.d.njmax, top.nconmax, top.njmax,
                        s->fast.spec, s->big.spec, s->ovf_cap, s->nrowclass};
  for (int i = 0; i < 8; i++) out[i] = v[i];
  return 0;
}

int mjx_launch_counts(int64_t* out, int n) {
  if (!out || n < 0) return fail("mjx_launch_counts: null output or negative length");
  std::vector<long long> v(n);
  mjx::launch_counts(v.data(), n);
  for (int i = 0; i < n; i++) out[i] = (int64_t)v[i];
  return 0;
}

int mjx_launch_counts_reset(void) {
  mjx::launch_counts_reset();
  mjx::sensor_ext_launches_reset();
  return 0;
}

int mjx_sensor_launch_count(int64_t* out) {
  if (!out) return fail("mjx_sensor_launch_count: null output");
  out[0] = (int64_t)mjx::sensor_ext_launches();
  return 0;
}

int mjx_marker(int tag, void* stream) {
  hipError_t e = mjx::launch_marker(tag, (hipStream_t)stream);
  if (e != hipSuccess) return fail(std::string("marker launch: ") + hipGetErrorString(e));
  return 0;
}

int mjx_sim_stats(mjxSim* s, int32_t* out, void* stream) {
  if (!s || !out) return fail("null argument");
  // per-world counters -> totals: [0] max contacts, [1] max rows, [2..4] overflow /
  // row-overflow / unsupported-pair events, [5] max Newton iterations
  std::vector<int32_t> ws((size_t)s->nworld * 8);
  HIPCHK(hipMemcpyAsync(ws.data(), s->dd.wstats, sizeof(int32_t) * ws.size(), hipMemcpyDeviceToHost,
                        (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  int32_t r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int w = 0; w < s->nworld; w++) {
    const int32_t* x = ws.data() + 8 * (size_t)w;
    r[0] = std::max(r[0], x[0]); r[1] = std::max(r[1], x[1]); r[5] = std::max(r[5], x[5]);
    r[2] += x[2]; r[3] += x[3]; r[4] += x[4];
  }
  // [6] overflow re-solves (worlds re-solved at the max capacity) over all worlds
  HIPCHK(hipMemcpyAsync(&r[6], s->dd.evtotal + 3, sizeof(int32_t), hipMemcpyDeviceToHost,
                        (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  for (int i = 0; i < 8; i++) out[i] = r[i];
  return 0;
}

}  // extern "C"
