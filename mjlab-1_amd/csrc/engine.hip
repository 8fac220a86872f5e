// engine.hip — host side of the mjx355 step engine for MI355X (gfx950): the generic step
// kernels (any model, dims read at run time), the reset kernel, kernel selection
// (generic vs model-specialised, specs.inc) and the launchers.  The kernels themselves are
// in engine_impl.h; spec.hip compiles them once per specs.inc entry.
#include "engine_impl.h"
#include "launch_select.h"

#include <atomic>
#include <vector>

namespace mjx {

// --------------------------------------------------------------------------- reset
__global__ void reset_kernel(Dims d, DModel m, DData D, const uint8_t* mask, int nworld,
                             int con_stride) {
  const int w = blockIdx.x;
  if (w >= nworld) return;
  if (mask && !mask[w]) return;
  const int lane = threadIdx.x;
  const float* qpos0 = m.qpos0 + (size_t)w * m.qpos0_ws;
  for (int i = lane; i < d.nq; i += blockDim.x) D.qpos[(size_t)w * d.nq + i] = qpos0[i];
  for (int i = lane; i < d.nv; i += blockDim.x) {
    size_t k = (size_t)w * d.nv + i;
    D.qvel[k] = 0; D.qacc_warmstart[k] = 0; D.qacc[k] = 0; D.qfrc_applied[k] = 0;
    D.qacc_smooth[k] = 0; D.qfrc_constraint[k] = 0;
  }
  for (int i = lane; i < d.nu; i += blockDim.x) {
    D.ctrl[(size_t)w * d.nu + i] = 0; D.actuator_force[(size_t)w * d.nu + i] = 0;
  }
  for (int i = lane; i < 6 * d.nbody; i += blockDim.x) D.xfrc_applied[(size_t)w * 6 * d.nbody + i] = 0;
  for (int i = lane; i < d.nsensordata; i += blockDim.x) D.sensordata[(size_t)w * d.nsensordata + i] = 0;
  for (int b = lane; b < d.nbody; b += blockDim.x) {
    int mid = m.body_mocapid[b];
    if (mid < 0) continue;
    const float* bp = m.body_pos + (size_t)w * m.body_pos_ws + 3 * b;
    const float* bq = m.body_quat + (size_t)w * m.body_quat_ws + 4 * b;
    for (int t = 0; t < 3; t++) D.mocap_pos[((size_t)w * d.nmocap + mid) * 3 + t] = bp[t];
    for (int t = 0; t < 4; t++) D.mocap_quat[((size_t)w * d.nmocap + mid) * 4 + t] = bq[t];
  }
  // contact output slots (mj_resetData: no contacts) up to the last output's reach, and the
  // output bookkeeping of engine_counters [6] / [7] with them (phase A's output trims to it)
  int* wsv = D.wstats + 8 * (size_t)w;
  const int nout = min(con_stride, max(wsv[6], wsv[7]));
  const size_t wc = (size_t)w * con_stride;
  for (int c = lane; c < nout; c += blockDim.x) {
    D.contact_dist[wc + c] = 0.f;
    D.contact_geom[(wc + c) * 2] = -1;
    D.contact_geom[(wc + c) * 2 + 1] = -1;
    for (int t = 0; t < 3; t++) D.contact_pos[(wc + c) * 3 + t] = 0.f;
    for (int t = 0; t < 9; t++) D.contact_frame[(wc + c) * 9 + t] = 0.f;
    for (int t = 0; t < 3; t++) D.contact_force[(wc + c) * 3 + t] = 0.f;
    if (m.max_condim > 3)  // (never written otherwise: zero since the allocation)
      for (int t = 0; t < 3; t++) m.contact_torque[(wc + c) * 3 + t] = 0.f;
  }
  __syncthreads();
  if (lane == 0) { D.time[w] = 0; D.ncon[w] = 0; D.nefc[w] = 0; wsv[6] = 0; wsv[7] = 0; }
}

// ------------------------------------------------------------------ Newton work lists
// One workgroup: counting sort of the worlds by constraint-row count (phase A's D.nefc),
// descending, then the segment of each row class.  Worlds outside `mask` are not listed.
// Order within equal row counts follows LDS atomics (each world's result is independent of
// it).
constexpr int kClassifyThreads = 1024;
constexpr int kMaxRowBins = 2048;
__global__ __launch_bounds__(kClassifyThreads) void classify_kernel(const Params* __restrict__ P,
                                                                    int w0, int w1, int split,
                                                                    const uint8_t* __restrict__ mask) {
  __shared__ int bin[kMaxRowBins];
  __shared__ int wsum[kClassifyThreads / kWave];
  constexpr int nwave = kClassifyThreads / kWave;
  const int nb = min(P->d.njmax + 1, kMaxRowBins);
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  for (int i = t; i < nb; i += kClassifyThreads) bin[i] = 0;
  __syncthreads();
  const int* nefc = P->D.nefc;
  // worlds listed for the overflow re-solve this substep (phase A left nefc = -1) are not
  // classed: the max launch set solves them
  for (int w = w0 + t; w < w1; w += kClassifyThreads) {
    const int r = nefc[w];
    if ((!mask || mask[w]) && r >= 0) atomicAdd(&bin[min(r, nb - 1)], 1);
  }
  __syncthreads();
  // exclusive scan of the bins in descending row count: bin[r] <- #listed worlds with more
  // than r rows.  Thread t owns a contiguous chunk of the reversed bin order.
  const int per = (nb + kClassifyThreads - 1) / kClassifyThreads;
  const int i0 = min(t * per, nb), i1 = min(i0 + per, nb);
  int run = 0;
  for (int i = i0; i < i1; i++) run += bin[nb - 1 - i];
  int x = run;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == kWave - 1) wsum[wv] = x;
  __syncthreads();
  if (wv == 0) {
    int v = lane < nwave ? wsum[lane] : 0;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int y = __shfl_up(v, o);
      if (lane >= o) v += y;
    }
    if (lane < nwave) wsum[lane] = v;  // inclusive over waves
  }
  __syncthreads();
  const int total = wsum[nwave - 1];
  int base = x - run + (wv > 0 ? wsum[wv - 1] : 0);
  for (int i = i0; i < i1; i++) {
    const int r = nb - 1 - i, c = bin[r];
    bin[r] = base;
    base += c;
  }
  __syncthreads();
  // row class k's segment: class 0 = rows > cap[nc-1] (the front of the list), class k >= 1
  // = rows in (cap[k-2], cap[k-1]] (class 1 from 0 rows)
  const int nc = P->nrowclass;
  if (t <= nc) {
    const int hi = t == 0 ? nb - 1 : min(P->row_cap[t - 1], nb - 1);
    const int lo = t == 0 ? (nc > 0 ? P->row_cap[nc - 1] : -1) : (t > 1 ? P->row_cap[t - 2] : -1);
    const int s0 = bin[hi];
    const int s1 = lo < 0 ? total : bin[min(lo, nb - 1)];
    // this split's list occupies wl_list[w0, w1): absolute segment starts
    int* seg = P->wl_seg + 2 * (kRowClasses + 1) * split;
    seg[2 * t] = w0 + s0;
    seg[2 * t + 1] = max(s1 - s0, 0);
  }
  __syncthreads();  // the segments read the bins before the scatter advances them
  for (int w = w0 + t; w < w1; w += kClassifyThreads) {
    const int r = nefc[w];
    if ((!mask || mask[w]) && r >= 0) P->wl_list[w0 + atomicAdd(&bin[min(r, nb - 1)], 1)] = w;
  }
}

// Generic kernels: one instantiation per (register-row length NR >= padded nv; phase), each
// NR in its own object (generic.hip with -DMJX_GENERIC_NR, compiled in parallel).
#define MJX_GENERIC_NRS(X) X(8) X(16) X(20) X(24) X(32) X(36) X(40) X(48) X(56) X(64)
#define MJX_DECL_GENERIC(nr) StepFn generic_fn_##nr(int ph);
MJX_GENERIC_NRS(MJX_DECL_GENERIC)
#undef MJX_DECL_GENERIC
static StepFn generic_fn(int nv, int ph) {
  // exact fits for the shipped robots (Go1 nvp 20, G1 nvp 36), multiples of 8 otherwise
  const int nvp = (nv + 3) & ~3;
  if (nvp <= 8) return generic_fn_8(ph);
  if (nvp <= 16) return generic_fn_16(ph);
  if (nvp <= 20) return generic_fn_20(ph);
  if (nvp <= 24) return generic_fn_24(ph);
  if (nvp <= 32) return generic_fn_32(ph);
  if (nvp <= 36) return generic_fn_36(ph);
  if (nvp <= 40) return generic_fn_40(ph);
  if (nvp <= 48) return generic_fn_48(ph);
  if (nvp <= 56) return generic_fn_56(ph);
  return generic_fn_64(ph);
}

// Model-specialised kernels (spec.hip, one object per specs.inc entry).
#define MJX_SPEC(id, scene, ...) StepFn spec_fn_##id(int ph);
#include "specs.inc"
#undef MJX_SPEC
// Run-time specialisations (jit.hip libraries, mjx_spec_register): ids kRtSpecBase + i.
struct RtSpec {
  Dims d;
  std::vector<int> par;
  StepFn (*fn)(int);
};
static std::vector<RtSpec>& rt_specs() {
  static std::vector<RtSpec> v;
  return v;
}
int register_spec(const Dims& d, const int* par, int npar, StepFn (*fn)(int)) {
  rt_specs().push_back(RtSpec{d, std::vector<int>(par, par + npar), fn});
  return kRtSpecBase + (int)rt_specs().size() - 1;
}
static StepFn spec_fn(int spec, int ph) {
  if (spec >= kRtSpecBase) {
    const int i = spec - kRtSpecBase;
    return i < (int)rt_specs().size() ? rt_specs()[i].fn(ph) : nullptr;
  }
  switch (spec) {
#define MJX_SPEC(id, scene, ...) case id: return spec_fn_##id(ph);
#include "specs.inc"
#undef MJX_SPEC
    default: return nullptr;
  }
}
static StepFn step_fn(const Params& host, PhaseCode ph, bool net) {
  const int code = net && phase_has_net(ph) ? ph | kPhNet : ph;
  StepFn f = host.spec > 0 ? spec_fn(host.spec, code) : nullptr;
  return f ? f : generic_fn(host.d.nv, code);
}
// ... with actuator networks bound, the variant whose phase A evaluates them
static StepFn step_fn(const Params& host, PhaseCode ph) {
  return step_fn(host, ph, host.act_on && host.net.nnet > 0);
}
// Launch counters (host side only; mjx_launch_counts): how many launches of each PhaseCode,
// and of classify_kernel (kLaunchClassify), this process has issued.  Counted
// where a launch is issued, not where step_fn looks a kernel up (look-ups also happen for
// kernels that are never launched), so a test of a launch variant can tell that its variant
// ran.  A captured graph's launches count once, at capture.
static std::atomic<long long> g_launches[kLaunchCounters];
void launch_counts(long long* out, int n) {
  for (int i = 0; i < n; i++)
    out[i] = i < kLaunchCounters ? g_launches[i].load(std::memory_order_relaxed) : 0;
}
void launch_counts_reset() {
  for (auto& c : g_launches) c.store(0, std::memory_order_relaxed);
}
// hipLaunchKernelGGL of the one-wave kernel `f`, counted under phase code `code`
#define MJX_LAUNCH(code, f, grid, lds, st, ...)                              \
  do {                                                                       \
    g_launches[code].fetch_add(1, std::memory_order_relaxed);                \
    hipLaunchKernelGGL(f, grid, dim3(kWave), lds, st, __VA_ARGS__);          \
  } while (0)
#define MJX_LAUNCH_CLASSIFY(st, ...)                                                       \
  do {                                                                                     \
    g_launches[kLaunchClassify].fetch_add(1, std::memory_order_relaxed);                   \
    hipLaunchKernelGGL(classify_kernel, dim3(1), dim3(kClassifyThreads), 0, st, __VA_ARGS__); \
  } while (0)
// The launch-time knobs (launch_select.h LaunchKnobs): read once, on first use, and cached for
// the life of the process.
static const LaunchKnobs& knobs() {
  static const LaunchKnobs k = read_launch_knobs([](const char* name) { return getenv(name); });
  return k;
}
// The worlds [w0, w1) of batch split k as a launch set takes them: the Params whose kernels and
// carves it uses (host copy for the launch geometry, device copy for the kernels) and the
// step's mask.
struct Worlds {
  const Params& host;
  const Params* dev;
  int k, w0, w1;
  const uint8_t* mask;
};
// One launch of phase code `code` for row class `cls` over W, a workgroup per world (or `grid`
// workgroups), its dynamic LDS from lds_need.  `arg`: the kernels' sixth argument (integrate
// for phases A and C and what holds them, the row class for a Newton launch).  step_fn never
// returns null for a phase code: the generic kernels stand in for every role.
static void launch(const Worlds& W, PhaseCode code, int cls, bool with_next_a, hipStream_t st,
                   int sel, int last, int arg, int grid = -1) {
  MJX_LAUNCH(code, step_fn(W.host, code), dim3(grid >= 0 ? grid : W.w1 - W.w0),
             lds_need(W.host, knobs(), code, cls, with_next_a), st, W.dev, W.w0, W.w1, sel, last,
             arg, W.mask);
}

int find_spec(const Dims& d, const int* dof_parentid) {
  if (const char* e = getenv("MJX355_NO_SPEC"))  // diagnostic: force the generic kernels
    if (atoi(e) != 0) return 0;
  auto eq = [](const Dims& a, const Dims& b) {
    return a.nq == b.nq && a.nv == b.nv && a.nu == b.nu && a.nbody == b.nbody &&
           a.njnt == b.njnt && a.ngeom == b.ngeom && a.nsite == b.nsite &&
           a.nsensor == b.nsensor && a.nsensordata == b.nsensordata && a.npair == b.npair &&
           a.nhfield == b.nhfield && a.nhfielddata == b.nhfielddata && a.nlevel == b.nlevel &&
           a.nchild == b.nchild && a.nmocap == b.nmocap && a.ngeom_lds == b.ngeom_lds &&
           a.npair_all == b.npair_all && a.nstatic == b.nstatic &&
           a.nstpartner == b.nstpartner && a.nboxbox == b.nboxbox && a.nconmax == b.nconmax && a.njmax == b.njmax;
  };
  // and the dof tree of the entry's tree-form SPD factors (rows_chol_tree)
  auto same_tree = [&](const int* par, int n) {
    if (n != d.nv) return false;
    for (int i = 0; i < n; i++)
      if (dof_parentid[i] != par[i]) return false;
    return true;
  };
#define MJX_SPEC(id, scene, ...) \
  if (eq(d, ModelSpec<id>::dims()) && same_tree(SpecTree<id>::par, SpecTree<id>::npar)) return id;
#include "specs.inc"
#undef MJX_SPEC
  for (int i = 0; i < (int)rt_specs().size(); i++) {
    const RtSpec& r = rt_specs()[i];
    if (eq(d, r.d) && same_tree(r.par.data(), (int)r.par.size())) return kRtSpecBase + i;
  }
  return 0;
}

// One-time kernel attributes: the dynamic-LDS limit of every step kernel whose launches can ask
// for more than the 64 KiB default, from the launches' own rule (lds_need).  The J-in-global
// Newton kernels never pass it (15,904 B at nv 64 and 256 rows, the largest the engine admits:
// tests/carve_invariants.cpp).  The chains also hold phases C and A, whose carve grows with the
// geoms that keep an LDS frame (152,176 B found among admitted models), and kPhNewtonLatCap the
// full fast carve (54,944 B at its default of at most 160 rows, 81,440 B at 256 rows when
// MJX355_HEAVY_CAP forces it).
hipError_t prepare_step(const Params& host) {
  for (int ph = 0; ph < kPhaseCodes; ph++) {
    const size_t need = lds_need_max(host, knobs(), PhaseCode(ph));
    // (networks are bound after the sim is made: their variants get the attribute here too)
    for (int net = 0; net < (phase_has_net(ph) ? 2 : 1); net++) {
      const StepFn f = step_fn(host, PhaseCode(ph), net != 0);
      if (need > 64 * 1024 && f) {
        hipError_t e = hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)need);
        if (e != hipSuccess) return e;
      }
    }
  }
  return hipSuccess;
}

// ------------------------------------------------------------------ batch split fork / join
// Batch split: the worlds in nsplit contiguous ranges, each range's A -> B -> C chain on its
// own stream (split 0 on the launch stream).  The ranges are independent, so one range's
// launches fill the tail of the other's (the last, partly filled round of workgroups per CU)
// and the launch gaps.  Measured: Go1 8192 worlds 4.91 -> 5.61 M env-steps/s at 2 splits (3:
// 5.47, 4: 5.38).  With row classes: launch_split_classes (flat fork / join); the default for
// those models is one split (capi.cpp).  Masked forwards (reset worlds) stay one launch set.
struct Splits {
  int n;
  int wb[kMaxSplit + 1];  // split k: worlds [wb[k], wb[k + 1])
  hipStream_t st[kMaxSplit];
};
static Splits make_splits(int nworld, int nsplit, hipStream_t stream, const SideStream* side) {
  Splits s;
  s.n = nsplit;
  for (int k = 0; k <= nsplit; k++) s.wb[k] = (int)(((long long)nworld * k) / nsplit);
  for (int k = 0; k < nsplit; k++) s.st[k] = k == 0 ? stream : side->split[k];
  return s;
}
// Fork: the split streams, and the first `nc` class streams of every split, wait for the
// launch stream.
static hipError_t fork_splits(const Splits& s, const SideStream* side, int nc) {
  hipError_t e = hipEventRecord(side->split_fork, s.st[0]);
  for (int k = 1; k < s.n && e == hipSuccess; k++) e = hipStreamWaitEvent(s.st[k], side->split_fork, 0);
  for (int k = 0; k < s.n; k++)
    for (int c = 0; c < nc && e == hipSuccess; c++)
      e = hipStreamWaitEvent(side->stream[k][c], side->split_fork, 0);
  return e;
}
// Join: the launch stream waits for those class streams, then for the split streams.
static hipError_t join_splits(const Splits& s, const SideStream* side, int nc) {
  hipError_t e = hipSuccess;
  for (int k = 0; k < s.n; k++)
    for (int c = 0; c < nc && e == hipSuccess; c++) {
      e = hipEventRecord(side->join[k][c], side->stream[k][c]);
      if (e == hipSuccess) e = hipStreamWaitEvent(s.st[0], side->join[k][c], 0);
    }
  for (int k = 1; k < s.n && e == hipSuccess; k++) {
    e = hipEventRecord(side->split_join[k], s.st[k]);
    if (e == hipSuccess) e = hipStreamWaitEvent(s.st[0], side->split_join[k], 0);
  }
  return e;
}

// Row class `cls` of W on stream cs, one substep: its Newton launch `ch`, then (piped) phase C
// and the next substep's phase A (`nx`) of the same worlds -- all in one launch (step_chain)
// where `ch` is chained.
static void issue_class(const Worlds& W, const LaunchChoice& ch, int cls, bool piped, hipStream_t cs,
                        int last, const NextSubstep& nx, int integrate) {
  const int csel = W.k | (cls + 1) << 8;
  if (ch.chained) {
    launch(W, ch.code, cls, !last, cs, csel | (last ? 0 : kSelChainA) | nx.chain_sel(), last, integrate);
    return;
  }
  launch(W, ch.code, cls, false, cs, W.k | ch.sel, last, cls);
  if (!piped) return;
  launch(W, kPhC, 0, false, cs, csel | ch.sel, last, integrate);
  if (!last) launch(W, kPhA, 0, false, cs, csel | nx.apar | ch.sel, nx.last, integrate);
}

// Batch split together with Newton row classes: every fork starts from the launch stream
// and every side stream joins back into it before the next fork ("flat" fork / join).  Per
// substep: [A of each split, classify] on the split streams, join; [each split's class
// chains (B, and piped C + next A) on the class streams, the smallest class on the split
// stream], join.  A fork from one side stream to another (split stream -> its class
// streams, the natural nesting) crashes hipStreamEndCapture under the HIP runtime torch
// bundles (a synthetic probe with no engine code reproduces it in a torch process and not
// standalone on ROCm 7.2: scripts/capture_probe*.{hip,py}), and the
// flat form keeps the capture to the fork / join shape the unsplit class path uses.
// A diagnostic topology: the plain class launches only (class_choice_plain), no overflow lists.
static hipError_t launch_split_classes(const Params& host, const Params* dev, int nsubstep,
                                       int integrate, const Splits& s, const SideStream* side,
                                       bool piped) {
  const int nc = host.nrowclass;
  hipError_t e = hipSuccess;
  for (int sub = 0; sub < nsubstep; sub++) {
    const int last = sub == nsubstep - 1;
    const NextSubstep nx{0, sub + 1 == nsubstep - 1};  // (no overflow lists: no parity bit)
    if ((e = fork_splits(s, side, 0)) != hipSuccess) return e;
    for (int k = 0; k < s.n; k++) {
      const Worlds W{host, dev, k, s.wb[k], s.wb[k + 1], nullptr};
      if (W.w1 <= W.w0) continue;
      if (!piped || sub == 0) launch(W, kPhA, 0, false, s.st[k], k, last, integrate);
      MJX_LAUNCH_CLASSIFY(s.st[k], dev, W.w0, W.w1, k, nullptr);
    }
    if ((e = join_splits(s, side, 0)) != hipSuccess || (e = fork_splits(s, side, nc)) != hipSuccess)
      return e;
    for (int k = 0; k < s.n; k++) {
      const Worlds W{host, dev, k, s.wb[k], s.wb[k + 1], nullptr};
      if (W.w1 <= W.w0) continue;
      for (int c = 0; c <= nc; c++) {  // classes 0, nc, nc - 1, ..., 2, then 1 on the split stream
        const int cls = c == 0 ? 0 : nc + 1 - c;
        issue_class(W, class_choice_plain(knobs(), cls), cls, piped,
                    c < nc ? side->stream[k][c] : s.st[k], last, nx, integrate);
      }
    }
    if ((e = join_splits(s, side, nc)) != hipSuccess) return e;
    if (piped) continue;
    if ((e = fork_splits(s, side, 0)) != hipSuccess) return e;
    for (int k = 0; k < s.n; k++) {
      const Worlds W{host, dev, k, s.wb[k], s.wb[k + 1], nullptr};
      if (W.w1 > W.w0) launch(W, kPhC, 0, false, s.st[k], k, last, integrate);
    }
    if ((e = join_splits(s, side, 0)) != hipSuccess) return e;
  }
  return hipGetLastError();
}

// Overflow re-solve chain of split k at substep `sub` (parity sub & 1): the listed worlds'
// substep at full capacity (step_resolve: max A, latency Newton, C), then -- when the class
// pipelines carry the next substep's phase A -- that phase A in the normal carve; the last
// of them empties the list on exit.  The grid is fixed (kOvfGrid workgroups, each looping
// over listed worlds); workgroups past the listed count exit at once.
static void ovf_chain(const Params& host, const Params* dev, const Params& hbig, const Params* dbig,
                      hipStream_t cs, int k, int w0, int w1, int sub, int nsubstep, int integrate,
                      bool next_a, bool in_line) {
  const int last = sub == nsubstep - 1;
  const int par = sub & 1;
  // the grid: kOvfGrid on a stream of its own (sized for heavy overflow; an empty list costs
  // the same at 1 or 256 workgroups there), kOvfGridInline where the chain runs in line on
  // the critical path (split batches: 256 max-carve workgroups per launch cost Go1 8 %;
  // engine.h kOvfGridInline); MJX355_OVF_GRID overrides both
  const int grid_env = knobs().ovf_grid;
  const int g = std::min(hbig.ovf_cap, grid_env > 0 ? grid_env : in_line ? kOvfGridInline : kOvfGrid);
  const int sel = k | kSelOvf | (par ? kSelRPar : 0);
  const bool next = next_a && !last;
  launch(Worlds{hbig, dbig, k, w0, w1, nullptr}, kPhResolve, 0, false, cs, sel | (next ? 0 : kSelClr),
         last, integrate, g);
  if (next) {
    const NextSubstep nx = next_substep(sub, nsubstep);
    launch(Worlds{host, dev, k, w0, w1, nullptr}, kPhOvfNextA, 0, false, cs, sel | kSelClr | nx.apar,
           nx.last, integrate, g);
  }
}

// Order of the concurrent branches in a captured graph.  Graph replay (ROCm 7 clr) keeps the
// first child of a fork on the launch queue and starts every further child on a parallel
// queue, whose start and join each wait on a cross-queue signal (kernel trace, G1 4,096:
// classify -> bulk chain 12 us on the parallel queue, 5.5 us in line).  So while capturing,
// the models without row classes capture their critical launch (the range chain, phase B)
// ahead of the re-solve chain's: Go1 flat 8,192 +1.2 %, rough Go1 +0.6 % (two interleaved
// rounds).  The row-class fork keeps its order (the full-capacity class first, on the launch
// queue): bulk chain first measured G1 2.94 -> 2.38 M, tracking 2.71 -> 2.19 M, since the
// full class's long-latency worlds then start behind the bulk chain's and end last.
// MJX355_MAIN_FIRST=0 / 1 forces it off / on.
static bool main_first(hipStream_t st) {
  const int mode = knobs().main_first;
  if (mode >= 0) return mode != 0;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}

// ------------------------------------------------------------------------------ launch_step
// What the launches of one launch_step call share, and one batch range at one substep.
struct StepCtx {
  const Params& host;
  const Params* dev;
  const Params* hbig;  // the max-capacity Params of the overflow re-solve, or null
  const Params* dbig;
  const SideStream* side;
  const uint8_t* mask;
  int nworld, nsubstep, integrate, nsplit;
  bool ovf;            // the re-solve chain runs (host.ovf_resolve, hbig and side present)
  bool piped;          // row classes: each class's C and next A behind its Newton (class_pipe)
  LaunchChoice flat;   // no row classes: the range's Newton launch or range chain
  MaskedChoice masked; // mask present: the masked forward's Newton launch
};
struct Range {
  Worlds W;
  hipStream_t st;
  int sub;
};
static void range_ovf_chain(const StepCtx& c, const Range& r, hipStream_t cs, bool next_a, bool in_line) {
  ovf_chain(c.host, c.dev, *c.hbig, c.dbig, cs, r.W.k, r.W.w0, r.W.w1, r.sub, c.nsubstep, c.integrate,
            next_a, in_line);
}
// The re-solve chain of a range on a stream of its own (side->ovf[k]): forked after the
// substep's phase A (and classify), joined at the end of the substep -- the empty chain
// overlaps the range's launches.  (Record the fork before the stream's next launch; launch
// the chain after it while capturing: main_first.)
static hipError_t ovf_fork_launch(const StepCtx& c, const Range& r, bool next_a) {
  hipError_t e = hipStreamWaitEvent(c.side->ovf[r.W.k], c.side->ovf_fork[r.W.k], 0);
  if (e == hipSuccess) range_ovf_chain(c, r, c.side->ovf[r.W.k], next_a, false);
  return e;
}
static hipError_t ovf_join(const StepCtx& c, const Range& r) {
  hipError_t e = hipEventRecord(c.side->ovf_join[r.W.k], c.side->ovf[r.W.k]);
  return e == hipSuccess ? hipStreamWaitEvent(r.st, c.side->ovf_join[r.W.k], 0) : e;
}

// The masked forward in the max carve (masked_choice): one launch, or A / latency Newton / C.
static hipError_t launch_masked_max(const StepCtx& c, hipStream_t stream) {
  const Worlds W{*c.hbig, c.dbig, 0, 0, c.nworld, c.mask};
  const LaunchChoice& ch = c.masked.newton;
  if (!ch.chained) launch(W, kPhA, 0, false, stream, 0, 1, c.integrate);
  launch(W, ch.code, 0, false, stream, 0, 1, ch.chained ? c.integrate : -1);
  if (!ch.chained) launch(W, kPhC, 0, false, stream, 0, 1, c.integrate);
  return hipGetLastError();
}

// One substep of a range with row classes, behind its phase A.  Row-class pipelines (one
// split): each class's Newton launch is followed on the same stream by its phase C and then by
// the next substep's phase A for the same worlds, so the bulk class's C and next A overlap the
// heavy class's Newton tail; the streams join before the next classify.  MJX355_CLASS_PIPE=0:
// phase C / A over every world after the join (diagnostic).
static hipError_t substep_classes(const StepCtx& c, const Range& r) {
  const Worlds& W = r.W;
  const int k = W.k, nc = c.host.nrowclass, last = r.sub == c.nsubstep - 1;
  hipError_t e = hipSuccess;
  if (c.mask) {
    // masked forward in the fast carve: one Newton launch over the masked worlds (masked_choice)
    launch(W, c.masked.newton.code, 0, false, r.st, k, last, -1);
    // (MJX355_MASKED_BIG=0) masked worlds past the fast carve: re-solved in line
    if (c.ovf) range_ovf_chain(c, r, r.st, false, true);
  } else {
    MJX_LAUNCH_CLASSIFY(r.st, c.dev, W.w0, W.w1, k, c.mask);
    // MJX355_OVF_STREAM=1 (diagnostic): the re-solve chain on a stream of its own, forked here
    // and joined after the class joins
    const bool ovf_own = c.ovf && knobs().ovf_stream;
    if (ovf_own && ((e = hipEventRecord(c.side->ovf_fork[k], r.st)) != hipSuccess ||
                    (e = ovf_fork_launch(c, r, c.piped)) != hipSuccess))
      return e;
    // Newton by row class, concurrently: the full-capacity class (few worlds, long
    // per-world latency) first on a side stream so its blocks dispatch first, the middle
    // classes on further side streams, the smallest (most worlds) on the launch stream.
    // Measured: forking the side classes after the smallest makes the full class the tail
    // (B span 240 -> 255 us, G1).
    if ((e = hipEventRecord(c.side->fork[k], r.st)) != hipSuccess) return e;
    const NextSubstep nx = next_substep(r.sub, c.nsubstep);
    auto issue = [&](hipStream_t cs, int cls) {
      issue_class(W, class_choice(knobs(), c.host.d.njmax, c.nworld, cls, c.piped), cls, c.piped, cs,
                  last, nx, c.integrate);
    };
    for (int i = 0; i < nc; i++) {
      hipStream_t cs = c.side->stream[k][i];
      if ((e = hipStreamWaitEvent(cs, c.side->fork[k], 0)) != hipSuccess) return e;
      issue(cs, i == 0 ? 0 : nc + 1 - i);  // 0, then nc, nc-1, ..., 2
      // the re-solve chain behind the full-capacity class (its stream ends well before the
      // bulk class's), not on a stream of its own: a further concurrent branch crashed
      // graph replay under torch's HIP runtime (two middle classes + the re-solve stream).
      // Measured ahead of that class instead: G1 -3 % (its 64 KiB workgroups then take
      // LDS from the bulk class's first Newton waves)
      if (i == 0 && c.ovf && !ovf_own) range_ovf_chain(c, r, cs, c.piped, false);
    }
    issue(r.st, 1);
    for (int i = 0; i < nc; i++) {
      e = hipEventRecord(c.side->join[k][i], c.side->stream[k][i]);
      if (e == hipSuccess) e = hipStreamWaitEvent(r.st, c.side->join[k][i], 0);
      if (e != hipSuccess) return e;
    }
    if (ovf_own && (e = ovf_join(c, r)) != hipSuccess) return e;
    if (c.piped) return hipSuccess;
  }
  launch(W, kPhC, 0, false, r.st, k, last, c.integrate);
  return hipSuccess;
}

// One substep of a range without row classes (Go1), behind its phase A: phase B and C, or the
// range's B -> C -> next substep's A as one launch (step_chain over every world of the range),
// as the class pipelines do for a class, when noclass_choice chose it.  Worlds listed for the
// re-solve skip the chain's B, C and A; the re-solve chain then runs their next A too.
// The re-solve chain runs on a stream of its own, or in line behind phase C on the split stream
// of a split batch (a fork from a split stream is a second-level fork, which breaks graph
// capture; capi.cpp).  Also in line behind a range chain on an unsplit batch: the chain's B, C
// and fused next A skip the listed worlds by ovf_flag[w], which the re-solve chain's next phase
// A rewrites, so a concurrent re-solve could clear a flag before the range chain's workgroup
// for that world reads it and the world would run one extra B -> C -> A.
static hipError_t substep_flat(const StepCtx& c, const Range& r) {
  const Worlds& W = r.W;
  const LaunchChoice& ch = c.flat;
  const int k = W.k, last = r.sub == c.nsubstep - 1;
  const bool in_line = c.ovf && (c.nsplit > 1 || ch.chained), forked = c.ovf && !in_line;
  const bool mfirst = main_first(r.st);
  hipError_t e = hipSuccess;
  if (forked && (e = hipEventRecord(c.side->ovf_fork[k], r.st)) != hipSuccess) return e;
  if (forked && !mfirst && (e = ovf_fork_launch(c, r, ch.chained)) != hipSuccess) return e;
  if (ch.chained)
    launch(W, ch.code, 0, !last, r.st,
           k | (last ? 0 : kSelChainA) | next_substep(r.sub, c.nsubstep).chain_sel(), last, c.integrate);
  else
    launch(W, ch.code, 0, false, r.st, k, last, 0);
  if (forked && mfirst && (e = ovf_fork_launch(c, r, ch.chained)) != hipSuccess) return e;
  if (!ch.chained) launch(W, kPhC, 0, false, r.st, k, last, c.integrate);
  if (in_line) range_ovf_chain(c, r, r.st, ch.chained, true);
  return forked ? ovf_join(c, r) : hipSuccess;
}

static hipError_t launch_phases(const Params& host, const Params* dev, int nworld, int nsubstep,
                                int integrate, const uint8_t* mask, hipStream_t stream,
                                const SideStream* side, const Params* hbig, const Params* dbig) {
  if (nworld <= 0) return hipSuccess;
  const LaunchKnobs& kn = knobs();
  const int nc = host.nrowclass;
  // (masked forwards stay one launch set)
  const int nsplit = (!mask && side) ? std::max(1, std::min(side->nsplit, kMaxSplit)) : 1;
  const StepCtx c{host, dev, hbig, dbig, side, mask, nworld, nsubstep, integrate, nsplit,
                  /*ovf=*/hbig && side && host.ovf_resolve,
                  /*piped=*/nc > 0 && !mask && kn.class_pipe,
                  noclass_choice(kn, side && side->range_chain, mask != nullptr),
                  masked_choice(kn, host.d.nhfield, nc, nworld, hbig != nullptr)};
  if (mask && c.masked.max_carve) return launch_masked_max(c, stream);
  if (nc > 0 && !side) return hipErrorInvalidValue;
  const Splits s = make_splits(nworld, nsplit, stream, side);
  if (nsplit > 1 && nc > 0) {
    // (diagnostic topology; the overflow re-solve is not wired into it)
    if (c.ovf) return hipErrorNotSupported;
    return launch_split_classes(host, dev, nsubstep, integrate, s, side, kn.class_pipe != 0);
  }
  hipError_t e = hipSuccess;
  if (nsplit > 1 && (e = fork_splits(s, side, 0)) != hipSuccess) return e;
  // the next substep's phase A runs behind this one's C (class pipelines, range chain)
  const bool next_a = c.piped || (nc == 0 && c.flat.chained);
  for (int sub = 0; sub < nsubstep; sub++) {
    const int last = sub == nsubstep - 1;
    const int apar = (sub & 1) ? kSelAPar : 0;  // phase A of this substep lists into parity sub & 1
    for (int k = 0; k < nsplit; k++) {
      const Range r{Worlds{host, dev, k, s.wb[k], s.wb[k + 1], mask}, s.st[k], sub};
      if (r.W.w1 <= r.W.w0) continue;
      if (!next_a || sub == 0) launch(r.W, kPhA, 0, false, r.st, k | apar, last, integrate);
      if ((e = nc > 0 ? substep_classes(c, r) : substep_flat(c, r)) != hipSuccess) return e;
    }
  }
  if ((e = join_splits(s, side, 0)) != hipSuccess) return e;
  return hipGetLastError();
}

// The step's launches, then -- on the launch stream, behind the last join -- the extended
// sensors of a model that has any (sensor_ext.hip): they read what the last substep stored.
hipError_t launch_step(const Params& host, const Params* dev, int nworld, int nsubstep,
                       int integrate, const uint8_t* mask, hipStream_t stream,
                       const SideStream* side, const Params* hbig, const Params* dbig,
                       const SensorExt* ext) {
  const hipError_t e = launch_phases(host, dev, nworld, nsubstep, integrate, mask, stream, side,
                                     hbig, dbig);
  if (e != hipSuccess || !ext || ext->n <= 0 || nworld <= 0) return e;
  return launch_sensor_ext(dev, *ext, nworld, mask, stream);
}

// One-wave workgroups resident per CU at `bytes` of dynamic LDS, as measured on MI355X
// (scripts/lds_occupancy.hip: the first-round workgroups of a grid of spinning waves).  The
// hardware fits fewer than 160 KiB / bytes: 13,184 B hold 11 per CU, not 12 (12 need
// <= 12,800 B), 14,560 B 10, not 11 (11 need <= 14,080 B), 16,384 B 9, 8,192 B 18.
int lds_residency(size_t bytes) {
  static const struct { size_t max_bytes; int per_cu; } kTable[] = {
      {8192, 18}, {10240, 16}, {11264, 14}, {12800, 12}, {14080, 11}, {15360, 10}, {16384, 9},
      {20480, 8}, {32768, 4}};
  for (const auto& t : kTable)
    if (bytes <= t.max_bytes) return t.per_cu;
  return bytes > 0 ? std::max(1, (int)((size_t)147456 / bytes)) : 32;
}

// The range chain runs phases A and C at the Newton kernel's residency (registers and the
// largest carve).  Measured (Go1, 24 / 96 carve, two ranges, two interleaved rounds on one
// box): flat 4,096 worlds (2,048 per range) 5.25 -> 5.60 M env-steps/s, rough 8,192 (4,096
// per range) 4.57 -> 4.82 M, flat 8,192 7.38 -> 7.07 M.  A range that fits one residency
// round of the chain gains (two launch ramps and gaps per substep go); so does a model with
// terrain collision, whose long per-world phase-A tails the chain's per-world flow absorbs;
// a flat range needing a second round loses the cheap phases' residency.
bool range_chain_default(const Params& host, int nworld, int nsplit) {
  const StepFn f = step_fn(host, kPhChain);
  hipFuncAttributes fa;
  if (!f || hipFuncGetAttributes(&fa, (const void*)f) != hipSuccess) return false;
  const int regs = (fa.numRegs + 7) & ~7;
  const int per_cu = std::min(4 * (regs > 0 ? std::min(8, 512 / regs) : 8),
                              lds_residency(lds_need(host, knobs(), kPhChain, 0, true)));
  int dev = 0, ncu = 256;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    ncu = 256;
  const int per_range = (nworld + std::max(nsplit, 1) - 1) / std::max(nsplit, 1);
  return per_range <= per_cu * ncu || host.d.nstatic > 0;
}

int choose_row_classes(const Dims& d, int spec, int (&caps)[kRowClasses]) {
  for (int k = 0; k < kRowClasses; k++) caps[k] = 0;
  int n = 0;
  if (const char* e = getenv("MJX355_ROW_CLASSES")) {  // diagnostic: "44,80" or "" (none)
    for (const char* c = e; *c && n < kRowClasses;) {
      const int v = atoi(c);
      if (v > 0 && v < d.njmax && (n == 0 || v > caps[n - 1])) caps[n++] = v;
      while (*c && *c != ',') c++;
      if (*c == ',') c++;
    }
    return n;
  }
  hipFuncAttributes fa;
  Params hp{};
  hp.d = d;
  hp.spec = spec;
  if (hipFuncGetAttributes(&fa, (const void*)step_fn(hp, kPhB)) != hipSuccess) return 0;
  // wave64 on gfx950: 512 VGPRs per SIMD lane (granule 8), 4 SIMDs per CU
  const int regs = (fa.numRegs + 7) & ~7;
  const int top = 4 * (regs > 0 ? std::min(8, 512 / regs) : 8);  // register-bound worlds/CU
  // largest row capacity (multiple of 4) whose phase-B carve lets `w` worlds share a CU
  auto cap_for = [&](int w) {
    Dims ds = d;
    for (int r = (d.njmax - 1) & ~3; r >= 8; r -= 4) {
      ds.njmax = r;
      if (lds_residency((size_t)make_lds(ds, 1).total * 4) >= w) return r;
    }
    return 0;
  };
  if (lds_residency((size_t)make_lds(d, 1).total * 4) >= top) return 0;  // no need
  // One class below the register-bound residency, the rest at full capacity (gated at 5/6 of
  // it).  Measured with the round-3 full-form Hessian (G1 4096, B span per substep): one class
  // at 44 / 52 / 60 / 64 / 72 / 84 rows 202 / 196 / 197 / 197 / 203 / 198 us; two classes
  // (44+84, 44+64, 60+100) 207-216 us -- concurrent class launches crowd each other out
  // A class that at most doubles the full carve's residency does not repay the classify
  // launch and the fork/join (Go1 8192: full carve 8 worlds/CU, B + gaps 136 -> 153 us)
  // Since the Newton Hessian is staged in LTR form (round 4: 60 rows 4052 -> 3476 words) the
  // class sits at 11/12 of the register-bound residency (G1: 64 rows, 11 worlds/CU).  G1
  // env-steps/s, caps default-5/6 (72 rows, 10/CU) / 56 (12/CU) / 64 (11/CU): velocity 4096
  // 2.636 / 2.662 / 2.657 M, jump flat 16384 7.80 / 7.80 / 7.88 M, jump hfield 16384 4.81 /
  // 4.88 / 4.87 M, rough 4096 2.45 / 2.46 / 2.47 M, tracking 2.46 / 2.47 / 2.46 M.
  const int full_per_cu = lds_residency((size_t)make_lds(d, 1).total * 4);
  for (int w : {(5 * top) / 6}) {
    if (w < 8 || 2 * full_per_cu > w) continue;
    const int r = cap_for((11 * top) / 12);
    if (r > 0 && (n == 0 || r > caps[n - 1]) && n < kRowClasses) caps[n++] = r;
  }
  return n;
}

// Profiling marker: an empty one-wave kernel whose dispatches bracket a region of interest
// in a kernel trace (mjx_marker; the argument is the tag, visible in the trace only by order).
__global__ void marker_kernel(int tag) {
  (void)tag;
}

hipError_t launch_marker(int tag, hipStream_t stream) {
  hipLaunchKernelGGL(marker_kernel, dim3(1), dim3(kWave), 0, stream, tag);
  return hipGetLastError();
}

hipError_t launch_reset(const Dims& d, const DModel& m, const DData& dd, const uint8_t* mask,
                        int nworld, int con_stride, hipStream_t stream) {
  if (nworld <= 0) return hipSuccess;
  hipLaunchKernelGGL(reset_kernel, dim3(nworld), dim3(kWave), 0, stream, d, m, dd, mask, nworld,
                     con_stride);
  return hipGetLastError();
}

}  // namespace mjx

