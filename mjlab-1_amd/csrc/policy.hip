// Rollout-time policy evaluation: rsl_rl's ActorCritic (observation normalisation, the actor
// and critic MLPs, the Gaussian draw, its log-probability) as one launch; mjx_policy_act of
// include/mjx355.h, bound by mjlab_amd/rl/fused_policy.py.
//
// Grid (ceil(n / 32), 2): blockIdx.y 0 is the actor, 1 the critic.  One 256-thread workgroup
// (4 waves, one per SIMD) carries 32 observation rows through every layer of its network;
// 4,096 envs are 128 row tiles x 2 networks = one workgroup per CU of an MI355X.
//
// Activations stay in LDS: two buffers of 32 rows ping-pong, the row stride the layer width
// rounded up to the k stage (32) plus 4 floats, so the 16-byte A reads of the 32 rows of a
// half wave fall on different banks.  The columns between the width and its rounding are
// written as zeros.  The normalised observation is staged into the first buffer, 512 columns
// at a time (an input of up to 1024 accumulates over two stagings), so that every layer is
// the same loop; the two buffers then never exceed 2 x 32 x 516 floats = 129 KB.
//
// A layer is D[32, nout] = X[32, K] W^T on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32
// accumulation).  The output columns are cut into tiles of 32; wave w owns tiles w, w + 4,
// w + 8, w + 12 (hidden widths are at most 512 = 16 tiles), each a 16-register accumulator;
// the layer body is compiled per number of tiles a wave owns (0..4).
// For the instruction lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]
// and receives D[8 (r >> 2) + 4 (l >> 5) + (r & 3)][l & 31] in register r.  Which k a slot
// carries is free as long as A and B agree, so a k stage is 32 columns: the half wave h = l >> 5
// takes columns 16 h .. 16 h + 15 of the stage and issue s of the 16 multiplies column 16 h + s.
// A lane's B operand of a stage is then 64 contiguous bytes of row j of W ([out, in] row-major
// as nn.Linear keeps it), the two halves together one 128-byte line: every line of W is fetched
// by one group of loads, straight from L2 into registers, four 16-byte loads per lane and tile
// (single dwords where the row length or the pointer is not a multiple of 16 bytes: the first
// layer).  The next stage's B (64 registers for four tiles) loads while the current stage's
// 64 multiplies (4,096 cycles) issue.  Every B load is unconditional -- past the row's end the
// address is clamped into the row and the value replaced by zero -- so that the wait before a
// stage's first multiply can leave the next stage's loads in flight (a load under a branch
// would force a wait for all of them).  Bias and activation are applied to the accumulators
// as they are written to the other LDS buffer.
//
// Tail: 8 threads per row.  Actor: a = mu + sigma eps, the log-probability summed over the
// row's columns by three shuffles.  Critic: the value.  Rows past n are clamped on load and
// skipped on store.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/mjx355.h"
#include "policy.h"

namespace {

constexpr int kRows = 32;      // rows per workgroup
constexpr int kThreads = 256;  // 4 waves
constexpr int kStage = 32;     // k columns per stage
constexpr int kChunk = 512;    // input columns staged at a time
constexpr int kMaxHidden = 512, kMaxInput = 1024, kMaxActions = 64;
constexpr size_t kMaxLds = 160 * 1024;

typedef float acc16 __attribute__((ext_vector_type(16)));

__host__ __device__ constexpr int round_up(int x, int m) { return (x + m - 1) / m * m; }
__host__ __device__ constexpr int lds_stride(int width) { return round_up(width, kStage) + 4; }

__device__ __forceinline__ float activate(float x, int kind) {
  switch (kind) {
    case 1: return fmaxf(x, 0.f);
    case 2: return x > 0.f ? x : expm1f(x);
    case 3: return tanhf(x);
    default: return x;
  }
}

// Columns [k, k + 16) of the row `row` (K floats) of W; zeros from column K on.  No branch:
// the addresses stay inside the row.
template <bool WIDE>
__device__ __forceinline__ void load_b(float (&b)[16], const float* __restrict__ row, int K, int k) {
  if (WIDE) {  // K and the row are multiples of 4 floats: a 16-byte group is inside the row or past it
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int kq = k + 4 * q;
      const float4 v = *reinterpret_cast<const float4*>(row + min(kq, K - 4));
      const bool in = kq < K;
      b[4 * q] = in ? v.x : 0.f, b[4 * q + 1] = in ? v.y : 0.f;
      b[4 * q + 2] = in ? v.z : 0.f, b[4 * q + 3] = in ? v.w : 0.f;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const float v = row[min(k + q, K - 1)];
      b[q] = k + q < K ? v : 0.f;
    }
  }
}

// Normalised observation columns [k_lo, k_lo + klen) of the tile's rows into `out`, zeros up
// to the stage.
__device__ __forceinline__ void stage_input(const mjxPolicyNet& net, int n, int row0, int k_lo,
                                            int klen, float* out, int sout, int tid) {
  const int kp = round_up(klen, kStage);
  const int wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r < kRows; r += kThreads / 64) {
    const int g = min(row0 + r, n - 1);
    const float* x = net.obs + (size_t)g * net.obs_stride + k_lo;
    for (int c = lane; c < kp; c += 64) {
      float v = 0.f;
      if (c < klen) {
        v = x[c];
        if (net.norm_mean) v = (v - net.norm_mean[k_lo + c]) / (net.norm_std[k_lo + c] + net.norm_eps);
      }
      out[r * sout + c] = v;
    }
  }
}

// One layer for a wave that owns NT column tiles: out = activation(in W^T + bias).  `in` and
// `out` are the two LDS buffers (row strides sin, sout); with STAGE the input is the
// observation, staged into `in` chunk by chunk.  Ends with the workgroup in step.
template <int NT, bool WIDE>
__device__ __forceinline__ void run_layer(const mjxPolicyNet& net, int l, bool stage, int n, int row0,
                                          float* in, int sin, float* out, int sout, int tid, int wave) {
  const int lane = tid & 63, half = lane >> 5;
  const int K = net.width[l], nout = net.width[l + 1];
  const float* __restrict__ W = net.weight[l];
  constexpr int NA = NT ? NT : 1;
  acc16 acc[NA];
  const float* wrow[NA];  // this lane's row of W per tile (its output column, clamped below nout)
#pragma unroll
  for (int t = 0; t < NT; t++) {
    wrow[t] = W + (size_t)min(32 * (wave + 4 * t) + (lane & 31), nout - 1) * K;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
  }
  const float* arow = in + (lane & 31) * sin + 16 * half;

  for (int k_lo = 0; k_lo < K; k_lo += kChunk) {
    const int klen = stage ? min(kChunk, K - k_lo) : K;
    if (stage) {
      if (k_lo) __syncthreads();  // the previous chunk's reads
      stage_input(net, n, row0, k_lo, klen, in, sin, tid);
      __syncthreads();
    }
    if (NT > 0) {
      const int nstage = (klen + kStage - 1) / kStage;
      float b0[NA][16], b1[NA][16];
      auto fetch = [&](float (&b)[NA][16], int s) {
#pragma unroll
        for (int t = 0; t < NT; t++) load_b<WIDE>(b[t], wrow[t], K, k_lo + s * kStage + 16 * half);
      };
      auto multiply = [&](const float (&b)[NA][16], int s) {
        float a[16];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          // 16-byte aligned: the strides and 16 * half are multiples of 4 floats
          const float4 v = *reinterpret_cast<const float4*>(
              __builtin_assume_aligned(arow + s * kStage + 4 * q, 16));
          a[4 * q] = v.x, a[4 * q + 1] = v.y, a[4 * q + 2] = v.z, a[4 * q + 3] = v.w;
        }
        const int left = klen - s * kStage;  // issue i carries columns i and 16 + i of the stage
#pragma unroll
        for (int i = 0; i < 16; i++) {
          if (i < left) {
#pragma unroll
            for (int t = 0; t < NT; t++)
              acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[t][i], acc[t], 0, 0, 0);
          }
        }
      };
      fetch(b0, 0);
      for (int s = 0; s < nstage; s += 2) {  // a fetch past the last stage reads clamped addresses
        fetch(b1, s + 1);
        multiply(b0, s);
        fetch(b0, s + 2);
        if (s + 1 < nstage) multiply(b1, s + 1);
      }
    }
    if (!stage) break;
  }
  // bias + activation on the accumulators, into the other buffer (zeros past nout)
  const int kind = l + 1 < net.nlayer ? net.activation : 0;
  const float* __restrict__ bias = net.bias[l];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int col = 32 * (wave + 4 * t) + (lane & 31);
    const bool in_range = col < nout;
    const float bv = bias[min(col, nout - 1)];
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int row = 8 * (r >> 2) + 4 * half + (r & 3);
      out[row * sout + col] = in_range ? activate(acc[t][r] + bv, kind) : 0.f;
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kThreads) k_policy_act(const mjxPolicyDesc d, int s0, int s1) {
  extern __shared__ __align__(16) float lds[];
  const bool is_critic = blockIdx.y != 0;
  const mjxPolicyNet& net = is_critic ? d.critic : d.actor;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * kRows, n = d.n;
  // buffer b of the ping-pong starts at lds + b * kRows * s0 (offsets, so that every access
  // stays an LDS instruction)
  const int second = kRows * s0;

  for (int l = 0; l < net.nlayer; l++) {
    const int K = net.width[l], ntile = (net.width[l + 1] + 31) / 32;
    const bool wide = (K & 3) == 0 && ((uintptr_t)net.weight[l] & 15) == 0;
    float* in = lds + ((l & 1) ? second : 0);
    float* out = lds + ((l & 1) ? 0 : second);
    const int sin = (l & 1) ? s1 : s0, sout = (l & 1) ? s0 : s1;
    const int nt = ntile > wave ? (ntile - wave + 3) / 4 : 0;  // tiles wave, wave + 4, ... < ntile
#define MJX_POLICY_LAYER(NT)                                                              \
  case NT:                                                                                \
    if (wide) run_layer<NT, true>(net, l, l == 0, n, row0, in, sin, out, sout, tid, wave); \
    else run_layer<NT, false>(net, l, l == 0, n, row0, in, sin, out, sout, tid, wave);     \
    break;
    switch (nt) {
      MJX_POLICY_LAYER(0)
      MJX_POLICY_LAYER(1)
      MJX_POLICY_LAYER(2)
      MJX_POLICY_LAYER(3)
      MJX_POLICY_LAYER(4)
    }
#undef MJX_POLICY_LAYER
  }

  // tail: 8 threads per row on the last layer's output
  const float* y = lds + ((net.nlayer & 1) ? second : 0);
  const int sy = (net.nlayer & 1) ? s1 : s0;
  const int row = tid >> 3, sub = tid & 7, g = row0 + row;
  const bool store = g < n;
  if (is_critic) {
    if (store && sub == 0 && d.values) d.values[(size_t)g * d.values_stride] = y[row * sy];
    return;
  }
  const int na = net.width[net.nlayer];
  if (!d.eps) {
    if (store && d.mu)
      for (int j = sub; j < na; j += 8) d.mu[(size_t)g * d.mu_stride + j] = y[row * sy + j];
    return;
  }
  float lp = 0.f;
  for (int j = sub; j < na; j += 8) {
    const float m = y[row * sy + j];
    const float sg = d.std_is_log ? expf(d.std[j]) : d.std[j];
    const float e = d.eps[(size_t)min(g, n - 1) * na + j];
    const float a = __fadd_rn(m, __fmul_rn(sg, e));  // two roundings, as mean + std * eps in torch
    const float dv = a - m;                          // torch's log_prob sees the rounded action
    lp += -(dv * dv) / (2.f * (sg * sg)) - logf(sg) - 0.918938533204672742f;
    if (store) {
      if (d.actions) d.actions[(size_t)g * d.actions_stride + j] = a;
      if (d.mu) d.mu[(size_t)g * d.mu_stride + j] = m;
      if (d.sigma) d.sigma[(size_t)g * d.sigma_stride + j] = sg;
    }
  }
  lp += __shfl_xor(lp, 1);
  lp += __shfl_xor(lp, 2);
  lp += __shfl_xor(lp, 4);
  if (store && sub == 0 && d.log_prob) d.log_prob[(size_t)g * d.log_prob_stride] = lp;
}

bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

// Empty when the network is within the kernel's limits.
std::string check_net(const mjxPolicyNet& net, const char* who, int max_out) {
  const std::string w = who;
  if (net.nlayer < 1 || net.nlayer > MJX_POLICY_MAX_LAYERS)
    return w + ": 1 <= nlayer <= " + std::to_string(MJX_POLICY_MAX_LAYERS);
  if (net.activation < 0 || net.activation > 3)
    return w + ": unknown activation " + std::to_string(net.activation) + " (0 none, 1 relu, 2 elu, 3 tanh)";
  if (net.width[0] < 1 || net.width[0] > kMaxInput)
    return w + ": input width must be in [1, " + std::to_string(kMaxInput) + "]";
  for (int l = 1; l < net.nlayer; l++)
    if (net.width[l] < 1 || net.width[l] > kMaxHidden)
      return w + ": hidden widths must be in [1, " + std::to_string(kMaxHidden) + "]";
  if (net.width[net.nlayer] < 1 || net.width[net.nlayer] > max_out)
    return w + ": output width must be in [1, " + std::to_string(max_out) + "]";
  for (int l = 0; l < net.nlayer; l++) {
    if (!net.weight[l] || !net.bias[l]) return w + ": null weight or bias";
    if (misaligned(net.weight[l]) || misaligned(net.bias[l])) return w + ": misaligned weight or bias";
  }
  if (!net.obs) return w + ": null obs";
  if (net.obs_stride < net.width[0]) return w + ": obs_stride below the input width";
  if (net.norm_mean && !net.norm_std) return w + ": norm_mean without norm_std";
  if (misaligned(net.obs) || misaligned(net.norm_mean) || misaligned(net.norm_std))
    return w + ": misaligned obs or normaliser";
  return "";
}

// LDS row strides of the two activation buffers: buffer l & 1 holds layer l's input.
void buffer_strides(const mjxPolicyNet& net, int* s) {
  for (int l = 0; l <= net.nlayer; l++) {
    const int width = l == 0 ? (net.width[0] < kChunk ? net.width[0] : kChunk) : net.width[l];
    if (lds_stride(width) > s[l & 1]) s[l & 1] = lds_stride(width);
  }
}

}  // namespace

namespace mjx {

int policy_act(const mjxPolicyDesc* d, hipStream_t stream, std::string* err) {
  if (!d) return *err = "null policy descriptor", -1;
  if (d->n <= 0) return *err = "policy: n must be positive", -1;
  const bool draw = d->eps != nullptr;
  const bool critic = draw && d->critic.nlayer != 0;
  *err = check_net(d->actor, "policy actor", kMaxActions);
  if (err->empty() && critic) *err = check_net(d->critic, "policy critic", 1);
  if (!err->empty()) return -1;
  if (draw && !d->std) return *err = "policy: null std", -1;
  if (critic && !d->values) return *err = "policy: a critic without a values output", -1;
  const void* ptrs[] = {d->std, d->eps, d->actions, d->values, d->log_prob, d->mu, d->sigma};
  for (const void* p : ptrs)
    if (misaligned(p)) return *err = "policy: misaligned pointer", -1;
  const int na = d->actor.width[d->actor.nlayer];
  if ((d->actions && d->actions_stride < na) || (d->mu && d->mu_stride < na) ||
      (d->sigma && d->sigma_stride < na) || (d->values && d->values_stride < 1) ||
      (d->log_prob && d->log_prob_stride < 1))
    return *err = "policy: output stride below the row width", -1;
  int s[2] = {0, 0};
  buffer_strides(d->actor, s);
  if (critic) buffer_strides(d->critic, s);
  const size_t lds = (size_t)kRows * (s[0] + s[1]) * sizeof(float);
  if (lds > kMaxLds) return *err = "policy: activations exceed the 160 KB LDS", -1;
  static bool lds_raised = false;  // once: the attribute holds for the process
  if (lds > 64 * 1024 && !lds_raised) {
    hipError_t e = hipFuncSetAttribute((const void*)k_policy_act,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    if (e != hipSuccess) return *err = std::string("policy LDS attribute: ") + hipGetErrorString(e), -1;
    lds_raised = true;
  }
  const dim3 grid((unsigned)((d->n + kRows - 1) / kRows), critic ? 2 : 1);
  hipLaunchKernelGGL(k_policy_act, grid, dim3(kThreads), lds, stream, *d, s[0], s[1]);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return *err = std::string("policy launch: ") + hipGetErrorString(e), -1;
  return 0;
}

}  // namespace mjx
