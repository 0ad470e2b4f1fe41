// mm_policy_gi_bank.hip -- K shared actor-critics of one shape on the K contiguous groups of one batch, forward fused with the
// action sample and the value (include/mm_policy_gi_bank.h).
//
// Every member is marl/single_agent/Model_gi.py:137-216 ActorCriticNetwork(state_split=True) at hidden 128, computed as
// policy_gi_kernel (mm_policy_gi.hip) computes it: the split gather into the 5 block-diagonal layer-1 tiles, fc2 160 -> 128 on
// f32-input MFMA with the activations in registers, the actor rows and the critic row as 64 FMAs per row per lane plus one
// cross-half add, log-softmax in fp32 in torch's order, the inverse-CDF sample of mm_sample_actions in fp64, written by h = 0.
// The sequence of floating-point operations of a row is policy_gi_kernel's, so a row's logp and value are bit-equal to
// mm_policy_gi_act's with the same weights.
//
// Whose weights a workgroup stages is policy_bank_kernel's scheme (mm_policy_bank.hip): a workgroup belongs to ONE group, found
// from the block prefix table; it stages that member's fragments once (about 92 KB of LDS, one workgroup per CU) and walks the
// group's tiles persistently.  Tiles are counted from the group's own start, so a group boundary need not be a multiple of 32;
// the row of obs / logp / value / actions and the sampler's key are the global agent index.  The group and block prefix tables
// ride in the by-value argument block, so a captured launch carries them and the host arrays are not read again.  The grid
// split is mm_policy_bank_grid's: this file has no arithmetic of its own for it.
#include "mm_policy_mfma.h"
#include "../../include/mm_policy_gi_bank.h"

namespace mm {
namespace gi_bank {
using namespace mfma;  // kHidden = 128: fc2 outputs (Model_gi hidden_size)

constexpr int kCat = 160;                      // hidden / 4 + hidden / 2 + hidden / 2
constexpr int kL1Steps = 3 + 4 * 5;            // A fragments of layer 1: fc11 3 k-steps, 4 tiles of fc12 / fc13 x 5
constexpr int kThreads = 64 * MM_BANK_WAVES;   // 8 waves = 2 per SIMD, as policy_gi_kernel
constexpr int kWaves = MM_BANK_WAVES;
constexpr uint32_t kDomain = 0x53414D50u;  // the sampler's Philox domain word (mm_sample_actions / mm_policy_act)
static_assert(MM_BANK_TILE == 32, "one wave per 32 agents: the MFMA tile");

struct Args {
  MMGiParams w;                                   // the twelve stacked bases
  long long group_start[MM_BANK_MAX_GROUPS + 1];  // entries past K hold n
  int block_start[MM_BANK_MAX_GROUPS + 1];        // entries past K hold the grid
};

__global__ __launch_bounds__(kThreads) void policy_gi_bank_kernel(const float *__restrict__ obs, int n_s, const Args a, int n_a,
                                                                  uint64_t seed, const uint64_t *__restrict__ counter,
                                                                  int32_t *__restrict__ actions, float *__restrict__ logp_out,
                                                                  float *__restrict__ value_out) {
  __shared__ float sW1[kL1Steps][64];   // [fragment][lane]: 5.75 KB
  __shared__ float4 sW2[4][20][64];     // [out tile][k-step / 4][lane]: 80 KB
  __shared__ float sWh[9][kHidden];     // actor_linear rows 0..7 (zero past n_a), critic_linear row 8: 4.5 KB
  __shared__ float sB1[kCat], sB2[kHidden], sBh[9];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  // ---- the workgroup's group: the last k whose block prefix is <= blockIdx (an empty group has no workgroup of its own)
  const int b = (int)blockIdx.x;
  int g = 0;
#pragma unroll
  for (int k = 1; k < MM_BANK_MAX_GROUPS; k++) g += a.block_start[k] <= b ? 1 : 0;
  const int lb = b - a.block_start[g], nb = a.block_start[g + 1] - a.block_start[g];
  const long long g0 = a.group_start[g], ng = a.group_start[g + 1] - g0;
  const float *__restrict__ W11 = a.w.W11 + g * 32 * 5;
  const float *__restrict__ b11 = a.w.b11 + g * 32;
  const float *__restrict__ W12 = a.w.W12 + g * 64 * 10;
  const float *__restrict__ b12 = a.w.b12 + g * 64;
  const float *__restrict__ W13 = a.w.W13 + g * 64 * 10;
  const float *__restrict__ b13 = a.w.b13 + g * 64;
  const float *__restrict__ W2 = a.w.W2 + g * kHidden * kCat;
  const float *__restrict__ b2 = a.w.b2 + g * kHidden;
  const float *__restrict__ Wa = a.w.Wa + g * n_a * kHidden;
  const float *__restrict__ ba = a.w.ba + g * n_a;
  const float *__restrict__ Wc = a.w.Wc + g * kHidden;
  const float *__restrict__ bc = a.w.bc + g;
  // ---- stage the member's weights in MFMA A-fragment order: A[i = l & 31][k = l >> 5] of step s is W[row][2 s + (l >> 5)]
  for (int t = tid; t < kL1Steps * 64; t += kThreads) {
    const int l = t & 63, q = t >> 6;
    int m, s;
    l1_step(q, m, s);
    const int k = 2 * s + (l >> 5);
    float w;
    if (m == 0) w = k < 5 ? W11[(l & 31) * 5 + k] : 0.0f;
    else if (m <= 2) w = W12[(32 * (m - 1) + (l & 31)) * 10 + k];
    else w = W13[(32 * (m - 3) + (l & 31)) * 10 + k];
    sW1[q][l] = w;
  }
  stage_w2<20, kThreads>(sW2, W2, kCat);
  for (int t = tid; t < 9 * kHidden; t += kThreads) {
    const int o = t / kHidden, c = t % kHidden;
    sWh[o][c] = o == 8 ? Wc[c] : (o < n_a ? Wa[o * kHidden + c] : 0.0f);
  }
  if (tid < 32) sB1[tid] = b11[tid];
  else if (tid < 96) sB1[tid] = b12[tid - 32];
  else if (tid < kCat) sB1[tid] = b13[tid - 96];
  if (tid < kHidden) sB2[tid] = b2[tid];
  if (tid < 9) sBh[tid] = tid == 8 ? bc[0] : (tid < n_a ? ba[tid] : 0.0f);
  __syncthreads();
  const bool sample = actions != nullptr;
  const uint64_t ctr = sample ? *counter : 0;
  const long long ntiles = (ng + 31) / 32;
  for (long long tile = (long long)lb * kWaves + wave; tile < ntiles; tile += (long long)nb * kWaves) {
    asm volatile("" ::: "memory");  // keep the tile-invariant LDS reads inside the persistent loop (mm_policy_mfma.h)
    const long long local = tile * 32 + j;
    const bool live = local < ng;
    const long long ag = g0 + local;  // the global agent index: the row of obs / logp / value / actions and the sampler's key
    const float *row = obs + (live ? ag : 0) * n_s;
    // B operands of layer 1, gathered by the split: input k = 2 s + h of each group
    float x1[3], x2[5], x3[5];
#pragma unroll
    for (int s = 0; s < 3; s++) {
      const int k = 2 * s + h;
      x1[s] = (live && k < 5) ? row[5 * k] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 5; s++) {
      const int k = 2 * s + h;
      x2[s] = live ? row[5 * (k >> 1) + 1 + (k & 1)] : 0.0f;
      x3[s] = live ? row[5 * (k >> 1) + 3 + (k & 1)] : 0.0f;
    }
    f32x16 h1[5], h2[4];
#pragma unroll
    for (int m = 0; m < 5; m++) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; r++) acc[r] = sB1[32 * m + frag_row(r, h)];
      if (m == 0) {
#pragma unroll
        for (int s = 0; s < 3; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sW1[s][lane], x1[s], acc, 0, 0, 0);
      } else {
        const int q0 = 3 + 5 * (m - 1);
#pragma unroll
        for (int s = 0; s < 5; s++)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sW1[q0 + s][lane], m <= 2 ? x2[s] : x3[s], acc, 0, 0, 0);
      }
      h1[m] = relu(acc);
    }
#pragma unroll
    for (int m = 0; m < 4; m++) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; r++) acc[r] = sB2[32 * m + frag_row(r, h)];
      h2[m] = relu(fc2_tile<5>(sW2[m], h1, lane, acc));
    }
    // ---- heads: actor rows 0..n_a-1, critic row 8
    float logit[8];
#pragma unroll
    for (int o = 0; o < 8; o++) {
      const float p = head_dot(h2, sWh[o], h, o < n_a);
      logit[o] = o < n_a ? p + sBh[o] : -INFINITY;
    }
    float v = 0.0f;
    if (value_out) {
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) v = fmaf(h2[m][r], sWh[8][32 * m + frag_row(r, h)], v);
      v = v + __shfl_xor(v, 32, 64);
    }
    const float mx = max8(logit);
    float se = 0.0f;
#pragma unroll
    for (int o = 0; o < 8; o++) se += exp_shifted(logit[o], mx, o < n_a);
    const float lg = logf(se);  // (logit - mx) - log(sum), as policy_kernel: the normaliser is not rounded at ulp(mx)
    if (live && h == 0) {
      if (value_out) value_out[ag] = v + sBh[8];
      double cdf[8], acc = 0;
#pragma unroll
      for (int o = 0; o < 8; o++) {
        const float lp = (logit[o] - mx) - lg;
        if (o < n_a) {
          if (logp_out) logp_out[ag * n_a + o] = lp;
          acc = acc + mmm_exp((double)lp);
          cdf[o] = acc;
        }
      }
      if (sample) {
        uint32_t w4[4];
        philox4x32((uint32_t)ag, (uint32_t)((uint64_t)ag >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32) ^ kDomain, (uint32_t)seed,
                   (uint32_t)(seed >> 32), w4);
        const double u = u53(w4[0], w4[1]);
        int act = 0;
#pragma unroll
        for (int o = 0; o < 8; o++)
          if (o < n_a) act += (cdf[o] / acc <= u) ? 1 : 0;  // searchsorted(cdf / cdf[-1], u, "right")
        actions[ag] = act < n_a - 1 ? act : n_a - 1;
      }
    }
  }
}

__global__ void counter_bump_kernel(uint64_t *counter) { *counter += 1; }

}  // namespace gi_bank
}  // namespace mm

extern "C" int32_t mm_policy_gi_bank_act(const float *obs, int64_t n, int32_t n_s, const MMGiParams *bank, int32_t K,
                                         const int64_t *group_start, int32_t hidden, int32_t n_a, uint64_t seed, uint64_t *counter,
                                         int32_t *actions, float *logp, float *value, MMStream stream) {
  using namespace mm::gi_bank;
  if (!obs || !mm::mfma::complete(bank)) return MM_ERR_INVALID_ARG;
  if (n < 0 || n_s < 25 || n_s > 32 || hidden != kHidden || n_a < 1 || n_a > 8) return MM_ERR_INVALID_ARG;
  if (!actions && !logp && !value) return MM_ERR_INVALID_ARG;
  if (actions && !counter) return MM_ERR_INVALID_ARG;
  Args a;
  // the group table's check (NULL, K, start at 0, non-decreasing) and the grid split are mm_policy_bank_act's
  if (mm_policy_bank_grid(K, group_start, a.block_start) != MM_OK || group_start[K] != n) return MM_ERR_INVALID_ARG;
  if (n == 0) return MM_OK;
  a.w = *bank;
  for (int k = 0; k <= MM_BANK_MAX_GROUPS; k++) {
    a.group_start[k] = group_start[k < K ? k : K];
    if (k > K) a.block_start[k] = a.block_start[K];
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(policy_gi_bank_kernel, dim3((unsigned)a.block_start[K]), dim3(kThreads), 0, s, obs, (int)n_s, a, (int)n_a, seed,
                     (const uint64_t *)counter, actions, logp, value);
  if (actions) hipLaunchKernelGGL(counter_bump_kernel, dim3(1), dim3(1), 0, s, counter);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
