// carve_invariants.cpp -- host program of tests/test_carve_invariants.py: what the step kernels
// (csrc/engine_impl.h) assume of the LDS carves of csrc/carve.h make_lds and nothing states,
// checked for every csrc/specs.inc entry and over a sweep of generic dims.  Prints one line
// per violated invariant (exit status 1), and at the end one summary line
//   dims <n> carves <n> failures <n> max_jg_bytes <b> max_chain_jg_bytes <b> max_cap_bytes <b>
//   max_cap256_bytes <b>
// with the largest dynamic LDS the launches of phase codes 9 / 10 (the J-in-global carve), 11
// (the full-capacity class's chain with J in global memory: the largest of that carve, phase
// C's and phase A's) and 12 (the full fast carve: at most 160 rows by default, any row
// capacity when MJX355_HEAVY_CAP forces it) can ask for over the models the engine admits
// (mjx_sim_create_ex: every phase carve within the CU's 160 KiB) -- what prepare_step
// (csrc/engine.hip) must raise the 64 KiB default of a kernel's dynamic LDS for.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "engine.h"

using mjx::Dims;
using mjx::Lds;
using mjx::make_lds;

static constexpr long kCuLds = 160 * 1024;
static long g_fail = 0, g_dims = 0, g_carves = 0;
static long g_max_jg = 0, g_max_chain_jg = 0, g_max_cap = 0, g_max_cap256 = 0;

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
  g_max_jg = std::max(g_max_jg, j);
  g_max_chain_jg = std::max(g_max_chain_jg, std::max(j, std::max(a, c)));
  if (d.njmax <= 160) g_max_cap = std::max(g_max_cap, b);
  g_max_cap256 = std::max(g_max_cap256, b);
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

int main() {
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
         "max_cap256_bytes %ld\n",
         g_dims, g_carves, g_fail, g_max_jg, g_max_chain_jg, g_max_cap, g_max_cap256);
  return g_fail ? 1 : 0;
}
