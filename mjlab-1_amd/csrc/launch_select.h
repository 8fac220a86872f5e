// launch_select.h — host-only decisions of launch_step (engine.hip): the launch-time
// MJX355_* knobs, which step kernel (phase code) and LDS carve a launch takes, and the dynamic
// LDS it asks for.  Pure functions of engine.h types: no HIP runtime calls, no statics, so
// tests/carve_invariants.cpp checks them with a plain host compiler.  Not shared with the
// kernels or the run-time specialisations (engine_impl.h does not include it).
#pragma once

#include <algorithm>
#include <cstdlib>

#include "engine.h"

namespace mjx {

// Launch-time knobs (A/B diagnostics), one field per MJX355_<NAME> variable; -1 = unset where
// the default depends on the model or the batch.  engine.hip reads them once per process, on
// first use.  INTEGRATION.md lists them for users; this struct is the source of truth.
struct LaunchKnobs {
  // NEWTON_LAT: the full-capacity Newton class and the masked forward run the latency kernel
  // (step_newton_lat); 0 keeps them on step_phase<NR, 1>.
  int newton_lat = 1;
  // HEAVY_CAP=0/1 forces heavy_cap() below off / on.
  int heavy_cap = -1;
  // NEWTON_JG: the full-capacity row class (the heavy worlds of the fast carve) reads the
  // constraint Jacobian from the B pack in global memory (carve kLdsJG) instead of an LDS copy.
  // 0 off, 1 the latency kernel (kPhNewtonLatJG), 2 the throughput kernel (kPhNewtonJG); with
  // CHAIN covering the full-capacity class, its chain (kPhChainLatJG).  Default: jg_mode().
  int newton_jg = -1;
  // CHAIN: which class chains run as one launch: 0 none, 1 every class, 2 the bulk class at any
  // batch size, 3 only the others.  Default: chain_on().
  int chain = -1;
  // OVF_GRID: workgroups of a re-solve launch, overriding kOvfGrid and kOvfGridInline (0: unset).
  int ovf_grid = 0;
  // OVF_STREAM=1 (diagnostic, scripts/capture_probe*): the re-solve chain of a row-class model
  // on a stream of its own, forked after classify and joined after the class joins -- round 4's
  // topology, kept to reproduce its graph-replay crash.
  int ovf_stream = 0;
  // MAIN_FIRST=0/1 forces the branch order of engine.hip main_first off / on.
  int main_first = -1;
  // MASKED_BIG=0/1 forces masked_max_carve() below.
  int masked_big = -1;
  // MASKED_FUSED=0: the max-carve masked forward as three launches instead of step_masked.
  int masked_fused = 1;
  // MASKED_JG=0: the fast-carve masked forward's Newton with J in LDS (masked_choice()).
  int masked_jg = 1;
  // CLASS_PIPE=0: phase C / next A over every world after the class join, instead of behind
  // each class's Newton launch on its stream (diagnostic).
  int class_pipe = 1;
  // RANGE_CHAIN=0/1 forces the range chain of a model without row classes (default:
  // range_chain_default, engine.hip).
  int range_chain = -1;
  // LDS_PAD=<bytes> (all phases) or LDS_PAD<ph>=<bytes> (phase 0/1/2) adds unused dynamic LDS
  // per world, to measure how throughput depends on resident worlds per CU.
  int lds_pad = 0, lds_pad_ph[3] = {0, 0, 0};
};

// `get`: const char* (const char* name), null when the variable is not set (getenv).
template <class Getenv>
LaunchKnobs read_launch_knobs(Getenv&& get) {
  auto num = [&](const char* name, int unset) {
    const char* e = get(name);
    return e ? atoi(e) : unset;
  };
  LaunchKnobs k;
  k.newton_lat = num("MJX355_NEWTON_LAT", 1) != 0;
  k.heavy_cap = num("MJX355_HEAVY_CAP", -1);
  k.newton_jg = num("MJX355_NEWTON_JG", -1);
  k.chain = num("MJX355_CHAIN", -1);
  k.ovf_grid = std::max(num("MJX355_OVF_GRID", 0), 0);
  k.ovf_stream = num("MJX355_OVF_STREAM", 0) != 0;
  k.main_first = num("MJX355_MAIN_FIRST", -1);
  k.masked_big = num("MJX355_MASKED_BIG", -1);
  k.masked_fused = num("MJX355_MASKED_FUSED", 1) != 0;
  k.masked_jg = num("MJX355_MASKED_JG", 1) != 0;
  k.class_pipe = num("MJX355_CLASS_PIPE", 1) != 0;
  k.range_chain = num("MJX355_RANGE_CHAIN", -1);
  k.lds_pad = num("MJX355_LDS_PAD", 0);
  k.lds_pad_ph[0] = num("MJX355_LDS_PAD0", 0);
  k.lds_pad_ph[1] = num("MJX355_LDS_PAD1", 0);
  k.lds_pad_ph[2] = num("MJX355_LDS_PAD2", 0);
  return k;
}

// ------------------------------------------------------------------------- dynamic LDS
// bytes of carve `c` (plus the diagnostic pad of its phase: every Newton carve pads as phase B)
inline size_t lds_bytes(const Params& host, const LaunchKnobs& kn, Carve c) {
  const int p = kn.lds_pad + kn.lds_pad_ph[c >= kCarveClass0 ? kCarveB : c];
  const Lds& L = c == kLdsJG ? host.LPJ : host.LP[c];
  return (size_t)L.total * 4 + (size_t)(p > 0 ? p : 0);
}
// the carve of a launch's Newton part: J in global memory for the codes that read it there, row
// class cls's carve for the throughput kernel and its chain (cls >= 1), the full carve otherwise
inline Carve newton_carve(PhaseCode code, int cls) {
  if (code == kPhNewtonLatJG || code == kPhNewtonJG || code == kPhChainLatJG) return kLdsJG;
  if ((code == kPhB || code == kPhChain) && cls > 0) return Carve(kCarveClass0 + cls - 1);
  return kCarveB;
}
// Dynamic LDS of one launch of `code` for row class `cls` (0: the full-capacity class, or no
// classes).  A chain holds its Newton carve, phase C's and, when it runs the next substep's
// phase A (with_next_a), phase A's; step_resolve and step_masked the largest of the three
// phase carves.  prepare_step raises a kernel's limit from this same function.
inline size_t lds_need(const Params& host, const LaunchKnobs& kn, PhaseCode code, int cls,
                       bool with_next_a) {
  const size_t a = lds_bytes(host, kn, kCarveA), c = lds_bytes(host, kn, kCarveC);
  const size_t b = lds_bytes(host, kn, newton_carve(code, cls));
  switch (code) {
    case kPhA: case kPhOvfNextA: return a;
    case kPhC: return c;
    case kPhResolve: case kPhMasked: return std::max(a, std::max(b, c));
    case kPhChain: case kPhChainLat: case kPhChainLatJG:
      return std::max(std::max(b, c), with_next_a ? a : (size_t)0);
    default: return b;  // the Newton kernels
  }
}

// The largest lds_need of `code` over the row classes and chain forms it can be launched with
// (a superset of them): what prepare_step raises the kernel's dynamic-LDS limit to.
inline size_t lds_need_max(const Params& host, const LaunchKnobs& kn, PhaseCode code) {
  size_t need = 0;
  for (int cls = 0; cls <= host.nrowclass; cls++)
    need = std::max(need, lds_need(host, kn, code, cls, true));
  return need;
}

// --------------------------------------------------------------------------- selection
// One Newton launch as launch_step issues it: the kernel, the carve of its Newton part, extra
// `sel` bits (kSelPrio; they also go to the piped C / next-A launches behind it), and whether
// it is a chain -- phase C and the next substep's phase A run inside it, none follow.
struct LaunchChoice {
  PhaseCode code;
  Carve carve;
  int sel;
  bool chained;
};
inline LaunchChoice choice(PhaseCode code, int cls, bool chained, int sel = 0) {
  return LaunchChoice{code, newton_carve(code, cls), sel, chained};
}

// Which class chains run as one launch (step_chain).  Default: the bulk class (class 1: the
// fewest rows, most worlds, on the launch stream) when the batch is at most kChainMaxWorlds.
// Measured (G1 4,096, two interleaved rounds on one box): bulk chained 2.81 M env-steps/s,
// every class chained 2.70 M, none 2.67 M, only the heavy classes 2.58 M -- the heavy class's
// latency kernel then runs its C and next A at one wave per SIMD; jump hfield at 16,384
// worlds (five residency rounds, whose per-slot sums already average the Newton tails):
// none 4.54 M, bulk 4.52 M, all 4.44 M.
constexpr int kChainMaxWorlds = 8192;
inline bool chain_on(const LaunchKnobs& kn, int cls, int nworld) {
  if (kn.chain < 0) return cls == 1 && nworld <= kChainMaxWorlds;
  return kn.chain == 1 || (kn.chain == 2 && cls == 1) || (kn.chain == 3 && cls != 1);
}
// J-in-global mode of the full-capacity class (LaunchKnobs::newton_jg): by default the
// throughput form past kChainMaxWorlds worlds, where that class holds thousands of worlds and
// its launch is throughput-bound by its LDS carve (jump hfield 16,384: ~5,400 worlds at 84-137
// rows, 4 per CU with J in LDS, 12 per CU without; 4.64 -> 4.80 M env-steps/s, two interleaved
// rounds), and off below (G1 4,096: ~670 heavy worlds, one per SIMD at most: +-0.5 %; tracking
// -1 %)
inline int jg_mode(const LaunchKnobs& kn, int nworld) {
  return kn.newton_jg >= 0 ? kn.newton_jg : nworld > kChainMaxWorlds ? 2 : 0;
}
// The full-capacity class's latency Newton kernel at the throughput kernels' 168 VGPRs
// (kPhNewtonLatCap; naturally ~193, 68 B per lane spilled when capped), its waves at raised issue
// priority (kSelPrio): a SIMD running a heavy world keeps two bulk-class waves beside it instead
// of one, and the heavy wave still issues first.  Measured (three interleaved rounds on one
// box): G1 velocity 4,096 +0.4 / +0.7 / +1.2 %, rough G1 +0.4 / +0.2 / +0.8 %; tracking (its
// 56 / 200 carve, heavy worlds up to ~190 rows) -0.7 / -0.3 / -0.6 %: on for fast carves of at
// most 160 rows.
inline bool heavy_cap(const LaunchKnobs& kn, int njmax) {
  return kn.heavy_cap >= 0 ? kn.heavy_cap != 0 : njmax <= 160;
}

// Row class `cls` of a model with row classes (0: the full-capacity class, 1: the bulk class).
// `piped`: the class's phase C and next phase A follow its Newton on its own stream
// (LaunchKnobs::class_pipe, no mask) -- as one launch where chain_on says so.
inline LaunchChoice class_choice(const LaunchKnobs& kn, int njmax, int nworld, int cls, bool piped) {
  const bool lat = kn.newton_lat != 0;
  const int jg = cls == 0 ? jg_mode(kn, nworld) : 0;
  if (piped && chain_on(kn, cls, nworld))
    return choice(cls == 0 && lat ? (jg == 1 ? kPhChainLatJG : kPhChainLat) : kPhChain, cls, true);
  if (cls != 0) return choice(kPhB, cls, false);
  if (jg == 1 && lat) return choice(kPhNewtonLatJG, 0, false);
  if (jg == 2) return choice(kPhNewtonJG, 0, false);
  if (lat && heavy_cap(kn, njmax)) return choice(kPhNewtonLatCap, 0, false, kSelPrio);
  return choice(lat ? kPhNewtonLat : kPhB, 0, false);
}
// ... and of the split-batch topology with row classes (launch_split_classes, diagnostic): no
// chains, J-in-global kernels or register cap
inline LaunchChoice class_choice_plain(const LaunchKnobs& kn, int cls) {
  return choice(cls == 0 && kn.newton_lat ? kPhNewtonLat : kPhB, cls, false);
}
// A batch range of a model without row classes: its B -> C -> next A as one launch (the range
// chain) where the knob or range_chain_default (`rchain_default`) chose it and no mask is
// present; else phase B (NEWTON_JG=2: J from global memory as well, A/B only).
inline LaunchChoice noclass_choice(const LaunchKnobs& kn, bool rchain_default, bool masked) {
  const bool rchain = kn.range_chain >= 0 ? kn.range_chain != 0 : rchain_default;
  if (rchain && !masked) return choice(kPhChain, 0, true);
  return choice(kn.newton_jg == 2 ? kPhNewtonJG : kPhB, 0, false);
}

// The masked forward (a few reset worlds): its launches in the max carve, or in the fast carve
// with the re-solve in line behind them.  The max-carve grid is the whole batch, and at 64 KiB
// of LDS per workgroup even the unmasked workgroups dispatch two per CU; the in-line re-solve
// is a fixed launch on the critical path.  Measured: G1 4,096 worlds max carve +1.1 %, jump
// hfield 16,384 worlds fast carve +9.5 % (round 6, two interleaved rounds: +14 %); round 6, max
// carve (fused, step_masked): Go1 8,192 +1.5 %, rough Go1 +2.0 %, jump flat 16,384 +0.8 %.  So
// the max carve unless a heightfield model has more than 4,096 worlds (its reset worlds' phase
// A at the max carve's 300 contacts is the slow part there).
inline bool masked_max_carve(const LaunchKnobs& kn, int nworld, int nhfield) {
  return kn.masked_big >= 0 ? kn.masked_big != 0 : nworld <= 4096 || nhfield == 0;
}
struct MaskedChoice {
  bool max_carve;       // the launches run in the max-capacity Params (hbig)
  LaunchChoice newton;  // kPhMasked: the whole forward as one launch; else between phases A and C
};
// Max carve (needs `hbig`): at full capacity throughout, nothing to re-solve; A -> B -> C as one
// launch (step_masked) unless MASKED_FUSED=0 (then the latency Newton kernel, whatever
// NEWTON_LAT says).  Fast carve with row classes: one Newton launch at full capacity over the
// masked worlds -- no classify launch, no fork/join latency on this short critical path.  Its
// grid is the whole batch and nearly every workgroup exits at once, so the launch costs its
// dispatch rounds: with J read from the B pack in global memory (carve kLdsJG, ~8 KB instead of
// the full fast carve's 31.8 KB) 16 workgroups fit a CU instead of 4 (MASKED_JG=0: J in LDS).
// Fast carve without row classes: as every other step of such a model, unchained.
inline MaskedChoice masked_choice(const LaunchKnobs& kn, int nhfield, int nrowclass, int nworld,
                                  bool hbig) {
  if (hbig && masked_max_carve(kn, nworld, nhfield))
    return {true, choice(kn.masked_fused ? kPhMasked : kPhNewtonLat, 0, kn.masked_fused != 0)};
  if (nrowclass == 0) return {false, noclass_choice(kn, false, true)};
  const bool lat = kn.newton_lat != 0;
  return {false, choice(lat ? (kn.masked_jg ? kPhNewtonLatJG : kPhNewtonLat) : kPhB, 0, false)};
}

// The substep after `sub` as a launch behind this one sees it: the parity of its overflow list
// as a `sel` bit, and whether it is the step's last (the `last` argument of a phase-A launch,
// kSelNextLast of a chain that runs that phase A itself).
struct NextSubstep {
  int apar;
  int last;
  int chain_sel() const { return apar | (last ? kSelNextLast : 0); }
};
inline NextSubstep next_substep(int sub, int nsubstep) {
  return NextSubstep{((sub + 1) & 1) ? kSelAPar : 0, sub + 1 == nsubstep - 1};
}

}  // namespace mjx
