// carve_invariants.cpp -- host program of tests/test_carve_invariants.py: what the step kernels
// (csrc/engine_impl.h) assume of the LDS carves of csrc/carve.h make_lds and nothing states,
// checked for every csrc/specs.inc entry and over a sweep of generic dims.  Prints one line
// per violated invariant (exit status 1), and at the end one summary line
//   dims <n> carves <n> failures <n> max_jg_bytes <b> max_chain_jg_bytes <b> max_cap_bytes <b>
//   max_cap256_bytes <b> launches <n>
// with the largest dynamic LDS (csrc/launch_select.h lds_need) the launches of phase codes 9 /
// 10 (the J-in-global carve), 11 (the full-capacity class's chain with J in global memory: the
// largest of that carve, phase C's and phase A's) and 12 (the full fast carve: at most 160
// rows by default, any row capacity when MJX355_HEAVY_CAP forces it) can ask for over the
// models the engine admits (mjx_sim_create_ex: every phase carve within the CU's 160 KiB) --
// what prepare_step (csrc/engine.hip) must raise the 64 KiB default of a kernel's dynamic LDS
// for.  Over the same sweep, every launch the selection functions of launch_select.h can
// return (any knob setting; `launches` of them) asks for no more than prepare_step's rule
// (lds_need_max) raises its kernel to; and the selection's known answers under default knobs.
//
// `carve_invariants select` instead prints the selection under the MJX355_* knobs of its
// environment for the topologies of tests/test_gpu_kernel_variants.py, as one line
//   cls0 <code> cls1 <code> masked_cls <code> masked_nocls <code> nocls <code>
// (one row class at 160 rows, piped unless MJX355_CLASS_PIPE=0; the masked forward with and
// without a row class; no row classes with the range chain chosen; all below 4,096 worlds
// with the max-capacity Params present).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "launch_select.h"

using namespace mjx;

static constexpr long kCuLds = 160 * 1024;
static long g_fail = 0, g_dims = 0, g_carves = 0;
static long g_max_jg = 0, g_max_chain_jg = 0, g_max_cap = 0, g_max_cap256 = 0;
static const LaunchKnobs kDefault{};

static std::string label(const Dims& d, const char* what) {
  char b[192];
  snprintf(b, sizeof b, "%s nv %d nbody %d nconmax %d njmax %d nhfield %d", what, d.nv, d.nbody,
           d.nconmax, d.njmax, d.nhfield);
  return b;
}
#define EXPECT(cond, d, what, ...)                                 \
  do {                                                             \
    if (!(cond)) {                                                 \
      g_fail++;                                                    \
      if (g_fail <= 40) {                                          \
        printf("FAIL %s: %s", label(d, what).c_str(), #cond);      \
        printf(" [" __VA_ARGS__);                                  \
        printf("]\n");                                             \
      }                                                            \
    }                                                              \
  } while (0)

static int pad4(int n) { return (n + 3) & ~3; }

// start of the first phase-B region outside the B pack (and outside the aliases into it:
// H, red, efc_Js and, where it fits, chol live in M's / efc_aref's pack slots)
static int first_nonpack(const Lds& L) {
  int lo = L.total;
  for (int o : {L.qacc_ws, L.x, L.Mx, L.srch, L.Ms, L.qfrc_con, L.efc_jar, L.efc_force, L.efc_act})
    lo = std::min(lo, o);
  if (L.chol != L.M) lo = std::min(lo, L.chol);
  return lo;
}

// the B carves of `d`: full, J in global memory, and a row class of `cap` rows each
static void check_b(const Dims& d, const std::vector<int>& caps) {
  const int nvp = pad4(d.nv), R = d.njmax;
  const Lds LB = make_lds(d, 1), LJ = make_lds(d, 1, true);
  g_carves += 2;
  // (1) the J-in-global carve keeps every pack offset up to efc_J
  EXPECT(LJ.ints == LB.ints, d, "jg", "%d %d", LJ.ints, LB.ints);
  EXPECT(LJ.M == LB.M, d, "jg", "%d %d", LJ.M, LB.M);
  EXPECT(LJ.qacc_smooth == LB.qacc_smooth, d, "jg", "%d %d", LJ.qacc_smooth, LB.qacc_smooth);
  EXPECT(LJ.qfrc_smooth == LB.qfrc_smooth, d, "jg", "%d %d", LJ.qfrc_smooth, LB.qfrc_smooth);
  EXPECT(LJ.efc_aref == LB.efc_aref, d, "jg", "%d %d", LJ.efc_aref, LB.efc_aref);
  EXPECT(LJ.efc_D == LB.efc_D, d, "jg", "%d %d", LJ.efc_D, LB.efc_D);
  EXPECT(LJ.efc_J == LB.efc_J, d, "jg", "%d %d", LJ.efc_J, LB.efc_J);
  EXPECT(mjx::jg_carve_agrees(d), d, "jg", "the static_assert's predicate");
  // the pack order the copies rely on: [ints M qacc_smooth qfrc_smooth efc_aref efc_D efc_J]
  for (const Lds* L : {&LB, &LJ}) {
    EXPECT(L->ints == 0 && L->ints + 8 <= L->M, d, "pack order", "%d %d", L->ints, L->M);
    // cp_pack(S, pack, L.M + ltr_size(nvp)): ints and M (LTR form) end before qacc_smooth
    EXPECT(L->M + mjx::ltr_size(nvp) <= L->qacc_smooth, d, "M slot", "%d %d", L->M, L->qacc_smooth);
    EXPECT(L->qacc_smooth + nvp <= L->qfrc_smooth, d, "pack order", "%d", L->qfrc_smooth);
    EXPECT(L->qfrc_smooth + nvp <= L->efc_aref, d, "pack order", "%d", L->efc_aref);
    EXPECT(L->efc_aref + pad4(R) <= L->efc_D, d, "pack order", "%d", L->efc_D);
    EXPECT(L->efc_D + pad4(R) <= L->efc_J, d, "pack order", "%d", L->efc_J);
  }
  // (2) the JG copy cp_pack(S + LJ.qacc_smooth, pack + LB.qacc_smooth, LB.efc_J - LB.qacc_smooth)
  // ends at or before the first region outside the pack, and inside the carve
  const int jg_end = LJ.qacc_smooth + (LB.efc_J - LB.qacc_smooth);
  EXPECT(jg_end <= first_nonpack(LJ), d, "jg copy", "%d %d", jg_end, first_nonpack(LJ));
  EXPECT(jg_end <= LJ.total && jg_end == LJ.pack_len, d, "jg copy", "%d %d %d", jg_end, LJ.total,
         LJ.pack_len);
  // ... and the full carve's copy of the pack with every row of J
  const int b_end = LB.efc_J + R * nvp;
  EXPECT(b_end <= first_nonpack(LB) && b_end <= LB.total, d, "full copy", "%d %d %d", b_end,
         first_nonpack(LB), LB.total);
  EXPECT(LJ.total <= LB.total, d, "jg size", "%d %d", LJ.total, LB.total);
  // (3) a class carve (Dims with njmax = the class capacity): [ints M qacc_smooth qfrc_smooth
  // efc_aref] at the full carve's offsets; efc_D and efc_J hold `cap` rows
  for (int cap : caps) {
    if (cap <= 0 || cap >= R) continue;
    Dims dc = d;
    dc.njmax = cap;
    const Lds LC = make_lds(dc, 1);
    g_carves++;
    EXPECT(LC.ints == LB.ints && LC.M == LB.M && LC.qacc_smooth == LB.qacc_smooth &&
               LC.qfrc_smooth == LB.qfrc_smooth && LC.efc_aref == LB.efc_aref,
           d, "class", "cap %d", cap);
    EXPECT(LC.M + mjx::ltr_size(nvp) <= LC.qacc_smooth, d, "class M slot", "cap %d", cap);
    EXPECT(LC.efc_aref + pad4(cap) <= LC.efc_D, d, "class efc_aref", "cap %d", cap);
    EXPECT(LC.efc_D + pad4(cap) <= LC.efc_J, d, "class efc_D", "cap %d", cap);
    EXPECT(LC.efc_J + cap * nvp <= first_nonpack(LC) && LC.efc_J + cap * nvp <= LC.total, d,
           "class efc_J", "cap %d: %d %d %d", cap, LC.efc_J + cap * nvp, first_nonpack(LC), LC.total);
    EXPECT(LC.total <= LB.total, d, "class size", "cap %d", cap);
  }
}

// Every (phase code, row class, chain runs the next phase A) launch_step can launch: the fixed
// launches, and whatever the selection functions return under any knob setting, batch size,
// row capacity and mask.
using Launch = std::tuple<int, int, bool>;
static const std::set<Launch>& reachable_launches() {
  static const std::set<Launch> all = [] {
    std::set<Launch> s;
    auto add = [&](const LaunchChoice& ch, int cls) {
      s.insert({ch.code, cls, false});
      if (ch.chained && ch.code != kPhMasked) s.insert({ch.code, cls, true});
    };
    for (PhaseCode c : {kPhA, kPhC, kPhOvfNextA, kPhResolve}) s.insert({c, 0, false});
    LaunchKnobs kn;
    for (kn.chain = -1; kn.chain <= 3; kn.chain++)
      for (kn.newton_jg = -1; kn.newton_jg <= 2; kn.newton_jg++)
        for (kn.heavy_cap = -1; kn.heavy_cap <= 1; kn.heavy_cap++)
          for (kn.newton_lat = 0; kn.newton_lat <= 1; kn.newton_lat++)
            for (int nworld : {64, 4096, 4097, 8192, 8193, 16384}) {
              for (int cls = 0; cls <= kRowClasses; cls++) {
                add(class_choice_plain(kn, cls), cls);
                for (int njmax : {64, 160, 164, 256})
                  for (bool piped : {false, true}) add(class_choice(kn, njmax, nworld, cls, piped), cls);
              }
              for (int m = 0; m < 12; m++) {  // range-chain knob x default x mask
                kn.range_chain = m / 4 - 1;
                add(noclass_choice(kn, m & 1, m & 2), 0);
              }
              for (int m = 0; m < 96; m++) {  // masked knobs x heightfield x row classes x hbig
                kn.masked_big = m / 32 - 1;
                kn.masked_fused = m & 1;
                kn.masked_jg = (m >> 1) & 1;
                add(masked_choice(kn, (m >> 2) & 1, (m >> 3) & 1, nworld, (m >> 4) & 1).newton, 0);
              }
            }
    return s;
  }();
  return all;
}

// phases A and C of `d`, the CU's LDS, and the dynamic LDS of the launches prepare_step
// (csrc/engine.hip) does not raise the 64 KiB default for
static void check_ac(const Dims& d, bool must_fit) {
  const Lds LA = make_lds(d, 0), LB = make_lds(d, 1), LC = make_lds(d, 2), LJ = make_lds(d, 1, true);
  g_carves += 4;
  g_dims++;
  // (4) phase C's pack: [every substep | the last substep's | phase B's part]
  EXPECT(0 < LC.packC_sub && LC.packC_sub <= LC.packC_b && LC.packC_b < LC.pack_len &&
             LC.pack_len <= LC.total,
         d, "C pack", "%d %d %d %d", LC.packC_sub, LC.packC_b, LC.pack_len, LC.total);
  EXPECT(LC.packC_b == LC.ints && LC.ints <= LC.efc_force && LC.efc_force <= LC.pack_len, d,
         "C pack", "%d %d %d", LC.ints, LC.efc_force, LC.pack_len);
  EXPECT(LC.qfrc_smooth + pad4(d.nv) == LC.packC_sub, d, "C pack", "%d %d", LC.qfrc_smooth,
         LC.packC_sub);
  // (5) no phase carve exceeds the CU's 160 KiB
  const long a = 4L * LA.total, b = 4L * LB.total, c = 4L * LC.total, j = 4L * LJ.total;
  const bool admitted = a <= kCuLds && b <= kCuLds && c <= kCuLds;  // mjx_sim_create_ex
  if (must_fit) EXPECT(admitted, d, "160 KiB", "%ld %ld %ld", a, b, c);
  if (!admitted) return;
  EXPECT(j <= kCuLds, d, "160 KiB jg", "%ld", j);
  // as launch_step sees the model: the Params' carves (capi.cpp host_params), two row classes
  Params P{};
  P.d = d;
  for (int i = 0; i < 3; i++) P.LP[i] = make_lds(d, i);
  P.LPJ = LJ;
  P.nrowclass = kRowClasses;
  for (int k = 0; k < kRowClasses; k++) {
    Dims dc = d;
    dc.njmax = std::max(4, (d.njmax * (k + 1) / (kRowClasses + 1)) & ~3);
    P.row_cap[k] = dc.njmax;
    P.LP[kCarveClass0 + k] = make_lds(dc, 1);
  }
  auto need = [&](PhaseCode code) { return (long)lds_need(P, kDefault, code, 0, true); };
  g_max_jg = std::max(g_max_jg, std::max(need(kPhNewtonLatJG), need(kPhNewtonJG)));
  g_max_chain_jg = std::max(g_max_chain_jg, need(kPhChainLatJG));
  if (heavy_cap(kDefault, d.njmax)) g_max_cap = std::max(g_max_cap, need(kPhNewtonLatCap));
  g_max_cap256 = std::max(g_max_cap256, need(kPhNewtonLatCap));
  // (6) prepare_step covers every launch: what it raises a kernel's dynamic LDS to is at least
  // what any launch of that kernel asks for past the 64 KiB default
  for (const Launch& l : reachable_launches()) {
    const PhaseCode code = PhaseCode(std::get<0>(l));
    const long n = (long)lds_need(P, kDefault, code, std::get<1>(l), std::get<2>(l));
    const long raised = (long)lds_need_max(P, kDefault, code);
    EXPECT(n <= 64 * 1024 || n <= raised, d, "prepare_step", "code %d cls %d next_a %d: %ld > %ld",
           std::get<0>(l), std::get<1>(l), (int)std::get<2>(l), n, raised);
    EXPECT(n <= kCuLds, d, "160 KiB launch", "code %d: %ld", std::get<0>(l), n);
  }
}

static Dims generic_dims(int nv, int ncon, int rows, bool hfield) {
  Dims d{};
  d.nv = nv;
  d.nq = nv + 1;
  d.nu = nv - 6;
  d.nbody = std::min(nv - 3, mjx::kMaxBodies);
  d.njnt = nv - 5;
  d.ngeom = 2 * nv + (hfield ? 1 : 0);
  d.ngeom_lds = 2 * nv;  // a heightfield keeps no LDS frame
  d.nsite = 6;
  d.nsensor = 9;
  d.nsensordata = 21;
  d.npair = d.npair_all = 4 * nv;
  d.nlevel = 8;
  d.nchild = d.nbody - 1;
  if (hfield) {
    d.nhfield = 1;
    d.nhfielddata = 4096;
    d.nstatic = 1;
    d.nstpartner = 8;
    d.npair_all += 8;
  }
  d.nconmax = ncon;
  d.njmax = rows;
  return d;
}

static long g_known_fail = 0;
#define KNOWN(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      g_known_fail++;                                            \
      printf("FAIL selection under default knobs: %s\n", #cond); \
    }                                                            \
  } while (0)
static bool is(const LaunchChoice& ch, PhaseCode code, Carve carve, int sel, bool chained) {
  return ch.code == code && ch.carve == carve && ch.sel == sel && ch.chained == chained;
}
// known answers of the selection with default knobs
static void check_known() {
  const LaunchKnobs kn;
  // one row class, 160 rows, piped
  KNOWN(is(class_choice(kn, 160, 4096, 0, true), kPhNewtonLatCap, kCarveB, kSelPrio, false));
  KNOWN(is(class_choice(kn, 160, 4096, 1, true), kPhChain, kCarveClass0, 0, true));
  KNOWN(is(class_choice(kn, 160, 16384, 0, true), kPhNewtonJG, kLdsJG, 0, false));
  KNOWN(is(class_choice(kn, 160, 16384, 1, true), kPhB, kCarveClass0, 0, false));
  KNOWN(is(class_choice(kn, 200, 4096, 0, true), kPhNewtonLat, kCarveB, 0, false));
  // the split-batch topology: codes 3 and 1 whatever the batch size
  KNOWN(is(class_choice_plain(kn, 0), kPhNewtonLat, kCarveB, 0, false));
  KNOWN(is(class_choice_plain(kn, 2), kPhB, Carve(kCarveClass0 + 1), 0, false));
  // masked forward with the max-capacity Params: one launch in the max carve ...
  for (int nc : {0, 1}) {
    KNOWN(masked_choice(kn, 0, nc, 16384, true).max_carve && masked_choice(kn, 1, nc, 4096, true).max_carve);
    KNOWN(is(masked_choice(kn, 0, nc, 16384, true).newton, kPhMasked, kCarveB, 0, true));
    KNOWN(is(masked_choice(kn, 1, nc, 4096, true).newton, kPhMasked, kCarveB, 0, true));
  }
  // ... unless a heightfield model has more than 4,096 worlds (or has no such Params)
  KNOWN(!masked_choice(kn, 1, 1, 4097, true).max_carve && !masked_choice(kn, 0, 1, 64, false).max_carve);
  KNOWN(is(masked_choice(kn, 1, 1, 4097, true).newton, kPhNewtonLatJG, kLdsJG, 0, false));
  KNOWN(is(masked_choice(kn, 1, 0, 4097, true).newton, kPhB, kCarveB, 0, false));
  // no row classes
  KNOWN(is(noclass_choice(kn, false, false), kPhB, kCarveB, 0, false));
  KNOWN(is(noclass_choice(kn, true, false), kPhChain, kCarveB, 0, true));
  KNOWN(is(noclass_choice(kn, true, true), kPhB, kCarveB, 0, false));
  LaunchKnobs jg2;
  jg2.newton_jg = 2;
  KNOWN(is(noclass_choice(jg2, false, false), kPhNewtonJG, kLdsJG, 0, false));
  // the next substep's sel bits
  KNOWN(next_substep(0, 4).apar == kSelAPar && next_substep(0, 4).last == 0 &&
        next_substep(1, 4).apar == 0 && next_substep(2, 4).chain_sel() == (kSelAPar | kSelNextLast));
  // the numbers are public (include/mjx355.h mjx_launch_counts)
  KNOWN(kPhNewtonLatCap == 12 && kPhaseCodes == 13 && kLaunchClassify == 13 && kLaunchCounters == 14 &&
        kLdsJG == 9);
}

static int print_selection() {
  const LaunchKnobs kn = read_launch_knobs([](const char* name) { return getenv(name); });
  const bool piped = kn.class_pipe != 0;
  printf("cls0 %d cls1 %d masked_cls %d masked_nocls %d nocls %d\n",
         class_choice(kn, 160, 96, 0, piped).code, class_choice(kn, 160, 96, 1, piped).code,
         masked_choice(kn, 1, 1, 64, true).newton.code, masked_choice(kn, 0, 0, 64, true).newton.code,
         noclass_choice(kn, true, false).code);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "select")) return print_selection();
  check_known();
  // every compiled specialisation, with every class capacity below its row capacity
#define MJX_SPEC(id, scene, ...)                                  \
  {                                                               \
    const Dims d{__VA_ARGS__};                                    \
    std::vector<int> caps;                                        \
    for (int c = 1; c < d.njmax; c++) caps.push_back(c);          \
    check_b(d, caps);                                             \
    check_ac(d, true);                                            \
  }
#include "specs.inc"
#undef MJX_SPEC
  // generic dims.  The B carves depend on nv and the row capacity only: every nv and row
  // capacity 8 .. 256, class capacities in steps of 4 (choose_row_classes) and a few of the
  // odd ones MJX355_ROW_CLASSES may name
  for (int nv = 6; nv <= 64; nv++)
    for (int rows = 8; rows <= 256; rows++) {
      std::vector<int> caps;
      for (int c = 4; c < rows; c += 4) caps.push_back(c);
      for (int c : {1, 7, rows / 2 + 1, rows - 1}) caps.push_back(c);
      check_b(generic_dims(nv, 48, rows, false), caps);
    }
  // phases A and C depend on the contact capacity and the geoms too
  for (int nv = 6; nv <= 64; nv++)
    for (int rows = 8; rows <= 256; rows += 8)
      for (int ncon = 4; ncon <= 64; ncon += 4)
        for (int hf = 0; hf < 2; hf++) check_ac(generic_dims(nv, ncon, rows, hf != 0), false);
  // models with many geoms that keep an LDS frame: phase A's carve (and with it a class
  // chain's dynamic LDS) grows by 12 words per geom while the model is still admitted
  for (int nv : {18, 35, 64})
    for (int ng : {256, 1024, 2048})
      for (int rows : {64, 160, 256})
        for (int ncon : {16, 48, 64}) {
          Dims d = generic_dims(nv, ncon, rows, false);
          d.ngeom = d.ngeom_lds = ng;
          check_ac(d, false);
        }
  printf("dims %ld carves %ld failures %ld max_jg_bytes %ld max_chain_jg_bytes %ld max_cap_bytes %ld "
         "max_cap256_bytes %ld launches %ld\n",
         g_dims, g_carves, g_fail + g_known_fail, g_max_jg, g_max_chain_jg, g_max_cap, g_max_cap256,
         (long)reachable_launches().size());
  return g_fail || g_known_fail ? 1 : 0;
}
