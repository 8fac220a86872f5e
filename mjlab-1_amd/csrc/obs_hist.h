// Observation history and delay of the fused observe kernels (mjxObsState,
// include/mjx355_task.h): the store of one frame element into its term's history block,
// through the term's delay ring, and the host-side checks of the segment tables.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/mjx355_task.h"

namespace mjxobs {

constexpr uint32_t D_LAG = 0x7000;  // draw id of a term's lag: D_LAG + group * MAX_OBS_TERMS + term

// Element i of group g's frame (value v, noise applied) of env e -> the group row `row`.
// `draw(id)` is the caller's counter-hash uniform in [0, 1) for (env, step, id).  Called by
// exactly one thread per (env, group, element); that thread alone touches column i - base of
// the term's ring and history block.
template <class Draw>
__device__ __forceinline__ void store(const mjxObsState& S, int g, float* __restrict__ row, int e,
                                      int nworld, int i, float v, Draw&& draw) {
  const mjxObsGroup& G = S.group[g];
  int s = 0, base = 0;
  while (s + 1 < G.nterm && i >= base + G.seg[s].width) base += G.seg[s++].width;
  const mjxObsSeg sg = G.seg[s];
  const int w = sg.width, j = i - base;
  if (sg.max_lag > 0) {
    // DelayBuffer.append + compute (delay_buffer.py:221-245), ring oldest first
    const int L = sg.max_lag + 1, p = S.delay_pushes[e];  // p: frames pushed before this one
    const int slot = g * MJX_TASK_MAX_OBS_TERMS + s;
    int lag = sg.min_lag;
    if (sg.max_lag > sg.min_lag)
      lag = min(sg.min_lag + (int)(draw(D_LAG + slot) * (float)(sg.max_lag - sg.min_lag + 1)), sg.max_lag);
    lag = min(lag, p);  // clamp to pushes - 1 after this push
    float* R = G.delay_ring[s] + (size_t)e * L * w + j;
    const float out = lag == 0 ? v : R[(L - lag) * w];  // read before the shift moves it down
    if (p == 0) {
      for (int l = 0; l < L; l++) R[l * w] = v;
    } else {
      for (int l = 0; l + 1 < L; l++) R[l * w] = R[(l + 1) * w];
      R[(L - 1) * w] = v;
    }
    if (j == 0) S.delay_lag[(size_t)slot * nworld + e] = lag;
    v = out;
  }
  float* blk = row + G.out_off[s] + j;
  const int H = sg.history;
  if (H <= 1) {
    *blk = v;
  } else if (S.fresh[e]) {
    for (int h = 0; h < H; h++) blk[h * w] = v;
  } else {
    for (int h = 0; h + 1 < H; h++) blk[h * w] = blk[(h + 1) * w];
    blk[(H - 1) * w] = v;
  }
}

// reset of env e's history / delay state (the managers' reset of the masked envs)
__device__ __forceinline__ void reset_env(const mjxObsState& S, int e, int nworld) {
  if (S.fresh) S.fresh[e] = 1;
  if (S.delay_pushes) {
    S.delay_pushes[e] = 0;
    for (int g = 0; g < 2; g++)
      for (int s = 0; s < S.group[g].nterm; s++)
        if (S.group[g].seg[s].max_lag > 0)
          S.delay_lag[(size_t)(g * MJX_TASK_MAX_OBS_TERMS + s) * nworld + e] = 0;
  }
}

// env e's frame is stored: the next observe appends (one thread per env, after every
// thread of the env has read the flag and the push count)
__device__ __forceinline__ void frame_done(const mjxObsState& S, int e) {
  if (S.fresh) S.fresh[e] = 0;
  if (S.delay_pushes) S.delay_pushes[e] = min(S.delay_pushes[e] + 1, 1 << 20);
}

inline bool enabled(const mjxObsState& S) { return S.group[0].nterm > 0 || S.group[1].nterm > 0; }

// Checks the tables against the task's layout and fills the derived fields (frame, out_off).
// `frame[g]`: elements of group g's single frame; `width[g]`: the descriptor's row width.
// Returns "" or the reason.
inline std::string prepare(mjxObsState& S, const int frame[2], const int width[2]) {
  char buf[200];
  if (!enabled(S)) {
    for (int g = 0; g < 2; g++)
      if (width[g] != frame[g]) {
        snprintf(buf, sizeof buf, "observation width %d of group %d does not match its layout (%d)",
                 width[g], g, frame[g]);
        return buf;
      }
    return "";
  }
  bool any_hist = false, any_delay = false;
  for (int g = 0; g < 2; g++) {
    mjxObsGroup& G = S.group[g];
    if (G.nterm < 1 || G.nterm > MJX_TASK_MAX_OBS_TERMS) {
      snprintf(buf, sizeof buf, "observation group %d: %d terms outside [1, %d]", g, G.nterm,
               MJX_TASK_MAX_OBS_TERMS);
      return buf;
    }
    int fsum = 0, off = 0;
    for (int s = 0; s < G.nterm; s++) {
      const mjxObsSeg& sg = G.seg[s];
      if (sg.width < 1) {
        snprintf(buf, sizeof buf, "observation group %d term %d: width %d", g, s, sg.width);
        return buf;
      }
      if (sg.history < 0 || sg.history > MJX_TASK_MAX_HISTORY) {
        snprintf(buf, sizeof buf, "observation group %d term %d: history %d outside [0, %d]", g, s,
                 sg.history, MJX_TASK_MAX_HISTORY);
        return buf;
      }
      if (sg.min_lag < 0 || sg.max_lag < sg.min_lag || sg.max_lag > MJX_TASK_MAX_LAG) {
        snprintf(buf, sizeof buf, "observation group %d term %d: lags [%d, %d] outside [0, %d]", g, s,
                 sg.min_lag, sg.max_lag, MJX_TASK_MAX_LAG);
        return buf;
      }
      if (sg.max_lag > 0 && !G.delay_ring[s]) {
        snprintf(buf, sizeof buf, "observation group %d term %d: delay without a ring buffer", g, s);
        return buf;
      }
      any_hist |= sg.history > 1;
      any_delay |= sg.max_lag > 0;
      G.out_off[s] = off;
      off += sg.width * (sg.history > 1 ? sg.history : 1);
      fsum += sg.width;
    }
    G.frame = fsum;
    if (fsum != frame[g] || off != width[g]) {
      snprintf(buf, sizeof buf,
               "observation group %d: segment table (frame %d, row %d) does not match the layout "
               "(frame %d) and width %d",
               g, fsum, off, frame[g], width[g]);
      return buf;
    }
  }
  if (any_hist && !S.fresh) return "observation history without the fresh-flag buffer";
  if (any_delay && (!S.delay_pushes || !S.delay_lag))
    return "observation delay without the push-count / lag buffers";
  return "";
}

}  // namespace mjxobs
