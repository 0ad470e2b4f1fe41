// mm_policy_gi.hip -- MAPPO_GI's shared actor-critic fused with the action sample (include/mm_policy_gi.h).
//
// marl/single_agent/Model_gi.py:137-216 ActorCriticNetwork(state_split=True), hidden 128, on f32-input MFMA in the transposed,
// one-wave-per-32-agents layout that mm_policy_mfma.h describes (it is policy_kernel's in mm_main.hip): an accumulator tile
// is directly the B operand of the next layer and activations never leave the register file.
//
//   layer 1  the three split linears as 5 block-diagonal output tiles: tile 0 = fc11 (32 outputs, K = 5 -> 3 k-steps of
//            2), tiles 1-2 = fc12 and tiles 3-4 = fc13 (K = 10 -> 5 k-steps each).  The split gather happens while the B
//            operand is loaded: k-step s of lane half h reads input k = 2 s + h of its group, i.e. observation column
//            5 (k >> 1) + 1 + (k & 1) (fc12), 5 (k >> 1) + 3 + (k & 1) (fc13), 5 k (fc11).  23 A fragments, 5.75 KB of LDS.
//            The 5 tiles in tile order are cat(out1, out2, out3): 160 features in 80 registers.
//   layer 2  fc2 160 -> 128: 4 output tiles x 80 k-steps, A fragments staged as 20 float4 groups per tile (80 KB of LDS,
//            one conflict-free ds_read_b128 per four MFMAs).
//   heads    actor_linear (n_a <= 8 rows) and critic_linear (1 row) as 64 FMAs per row per lane plus one cross-half add,
//            then log-softmax (fp32), the value, and the inverse-CDF sample (fp64) of mm_sample_actions, written by h = 0.
#include "mm_policy_mfma.h"
#include "../../include/mm_policy_gi.h"

namespace mm {
namespace gi {
using namespace mfma;  // kHidden = 128: fc2 outputs (Model_gi hidden_size)

constexpr int kCat = 160;                  // hidden / 4 + hidden / 2 + hidden / 2
constexpr int kL1Steps = 3 + 4 * 5;        // A fragments of layer 1: fc11 3 k-steps, 4 tiles of fc12 / fc13 x 5
constexpr int kThreads = 512;              // 8 waves = 2 per SIMD, as policy_kernel
constexpr uint32_t kDomain = 0x53414D50u;  // the sampler's Philox domain word (mm_sample_actions / mm_policy_act)

__global__ __launch_bounds__(kThreads) void policy_gi_kernel(
    const float *__restrict__ obs, long long n, int n_s, const float *__restrict__ W11, const float *__restrict__ b11,
    const float *__restrict__ W12, const float *__restrict__ b12, const float *__restrict__ W13, const float *__restrict__ b13,
    const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ Wa, const float *__restrict__ ba,
    const float *__restrict__ Wc, const float *__restrict__ bc, int n_a, uint64_t seed, const uint64_t *__restrict__ counter,
    int32_t *__restrict__ actions, float *__restrict__ logp_out, float *__restrict__ value_out) {
  __shared__ float sW1[kL1Steps][64];   // [fragment][lane]: 5.75 KB
  __shared__ float4 sW2[4][20][64];     // [out tile][k-step / 4][lane]: 80 KB
  __shared__ float sWh[9][kHidden];     // actor_linear rows 0..7 (zero past n_a), critic_linear row 8: 4.5 KB
  __shared__ float sB1[kCat], sB2[kHidden], sBh[9];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  // ---- stage the weights in MFMA A-fragment order: A[i = l & 31][k = l >> 5] of step s is W[row][2 s + (l >> 5)]
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
  const long long ntiles = (n + 31) / 32;
  constexpr int kWaves = kThreads / 64;
  for (long long tile = (long long)blockIdx.x * kWaves + wave; tile < ntiles; tile += (long long)gridDim.x * kWaves) {
    asm volatile("" ::: "memory");  // keep the tile-invariant LDS reads inside the persistent loop (mm_policy_mfma.h)
    const long long ag = tile * 32 + j;
    const bool live = ag < n;
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
        int a = 0;
#pragma unroll
        for (int o = 0; o < 8; o++)
          if (o < n_a) a += (cdf[o] / acc <= u) ? 1 : 0;  // searchsorted(cdf / cdf[-1], u, "right")
        actions[ag] = a < n_a - 1 ? a : n_a - 1;
      }
    }
  }
}

__global__ void counter_bump_kernel(uint64_t *counter) { *counter += 1; }

}  // namespace gi
}  // namespace mm

extern "C" int32_t mm_policy_gi_act(const float *obs, int64_t n, int32_t n_s, const float *W11, const float *b11, const float *W12,
                                    const float *b12, const float *W13, const float *b13, const float *W2, const float *b2,
                                    const float *Wa, const float *ba, const float *Wc, const float *bc, int32_t hidden, int32_t n_a,
                                    uint64_t seed, uint64_t *counter, int32_t *actions, float *logp, float *value, MMStream stream) {
  using namespace mm::gi;
  if (!obs || !W11 || !b11 || !W12 || !b12 || !W13 || !b13 || !W2 || !b2 || !Wa || !ba || !Wc || !bc) return MM_ERR_INVALID_ARG;
  if (n < 0 || n_s < 25 || n_s > 32 || hidden != kHidden || n_a < 1 || n_a > 8) return MM_ERR_INVALID_ARG;
  if (!actions && !logp && !value) return MM_ERR_INVALID_ARG;
  if (actions && !counter) return MM_ERR_INVALID_ARG;
  if (n == 0) return MM_OK;
  hipStream_t s = (hipStream_t)stream;
  const long long ntiles = (n + 31) / 32;
  const unsigned grid = persistent_grid(ntiles, kThreads / 64);
  hipLaunchKernelGGL(policy_gi_kernel, dim3(grid), dim3(kThreads), 0, s, obs, (long long)n, (int)n_s, W11, b11, W12, b12, W13, b13,
                     W2, b2, Wa, ba, Wc, bc, (int)n_a, seed, (const uint64_t *)counter, actions, logp, value);
  if (actions) hipLaunchKernelGGL(counter_bump_kernel, dim3(1), dim3(1), 0, s, counter);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
