// mm_policy_bank.hip -- K actors of one shape on the K contiguous groups of one batch, forward fused with the action sample
// (include/mm_policy_bank.h).
//
// Every member is marl/single_agent/Model_common.py:5-22 ActorNetwork at hidden 128, computed as policy_kernel (mm_main.hip)
// computes it: on f32-input MFMA in the transposed, one-wave-per-32-agents layout that mm_policy_mfma.h describes, activations in
// registers, layer 3 as 64 FMAs per row per lane plus one cross-half add, log-softmax in fp32 in torch's order, the inverse-CDF
// sample of mm_sample_actions in fp64, written by h = 0.  The sequence of floating-point operations of a row is policy_kernel's,
// so a row's logp is bit-equal to mm_policy_act's with the same weights.
//
// What is new is whose weights a workgroup stages.  A workgroup belongs to ONE group: it finds its group from the block prefix
// table, stages that member's fragments once (84 KB of LDS, one workgroup per CU) and walks the group's tiles persistently.  Tiles
// are counted from the group's own start, so a group boundary need not be a multiple of 32; the sampler is keyed on the global
// agent index.  The group and block prefix tables ride in the by-value argument block (a uniform lookup: scalar loads from
// the kernel-argument segment), so a captured launch carries them and the host arrays are not read again.
//
// The grid split (bank_grid, host): the 256 persistent workgroups are divided over the non-empty groups in proportion to their
// tiles, rounded down, never more than a group has tile octets and never fewer than one; what the rounding leaves over goes, one
// workgroup at a time, to the group with the most tiles per workgroup.  At most 256 + K workgroups in all.
#include "mm_policy_mfma.h"
#include "../../include/mm_policy_bank.h"

namespace mm {
namespace bank {
using namespace mfma;  // kHidden = 128

constexpr int kThreads = 64 * MM_BANK_WAVES;  // 8 waves = 2 per SIMD, as policy_kernel
constexpr int kWaves = MM_BANK_WAVES;
constexpr uint32_t kDomain = 0x53414D50u;  // the sampler's Philox domain word (mm_sample_actions / mm_policy_act)
static_assert(MM_BANK_TILE == 32, "one wave per 32 agents: the MFMA tile");

struct Args {
  MMMlpParams w;                                 // the six stacked bases
  long long group_start[MM_BANK_MAX_GROUPS + 1];  // entries past K hold n
  int block_start[MM_BANK_MAX_GROUPS + 1];        // entries past K hold the grid
};

__global__ __launch_bounds__(kThreads) void policy_bank_kernel(const float *__restrict__ obs, int n_s, const Args a, int n_a,
                                                               uint64_t seed, const uint64_t *__restrict__ counter,
                                                               int32_t *__restrict__ actions, float *__restrict__ logp_out) {
  __shared__ float4 sW1[4][4][64];   // [out tile][k-step / 4][lane]: 16 KB
  __shared__ float4 sW2[4][16][64];  // 64 KB
  __shared__ float sW3[8][kHidden];
  __shared__ float sB1[kHidden], sB2[kHidden], sB3[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  // ---- the workgroup's group: the last k whose block prefix is <= blockIdx (an empty group has no workgroup of its own)
  const int b = (int)blockIdx.x;
  int g = 0;
#pragma unroll
  for (int k = 1; k < MM_BANK_MAX_GROUPS; k++) g += a.block_start[k] <= b ? 1 : 0;
  const int lb = b - a.block_start[g], nb = a.block_start[g + 1] - a.block_start[g];
  const long long g0 = a.group_start[g], ng = a.group_start[g + 1] - g0;
  const float *__restrict__ W1 = a.w.W1 + (long long)g * kHidden * n_s;
  const float *__restrict__ b1 = a.w.b1 + g * kHidden;
  const float *__restrict__ W2 = a.w.W2 + g * kHidden * kHidden;
  const float *__restrict__ b2 = a.w.b2 + g * kHidden;
  const float *__restrict__ W3 = a.w.W3 + g * n_a * kHidden;
  const float *__restrict__ b3 = a.w.b3 + g * n_a;
  // ---- stage the member's weights in MFMA A-fragment order: A[i = l & 31][k = l >> 5] of step s is W[32 m + i][k(s, h)]
  for (int t = tid; t < 4 * 4 * 64; t += kThreads) {
    const int l = t & 63, q = (t >> 6) & 3, m = t >> 8;
    float w[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = frag_row(4 * q + u, l >> 5);
      w[u] = k < n_s ? W1[(32 * m + (l & 31)) * n_s + k] : 0.0f;
    }
    sW1[m][q][l] = make_float4(w[0], w[1], w[2], w[3]);
  }
  stage_w2<16, kThreads>(sW2, W2, kHidden);
  for (int t = tid; t < 8 * kHidden; t += kThreads) sW3[t / kHidden][t % kHidden] = (t / kHidden) < n_a ? W3[t] : 0.0f;
  if (tid < kHidden) { sB1[tid] = b1[tid]; sB2[tid] = b2[tid]; }
  if (tid < 8) sB3[tid] = tid < n_a ? b3[tid] : 0.0f;
  __syncthreads();
  const uint64_t ctr = *counter;
  const long long ntiles = (ng + 31) / 32;
  for (long long tile = (long long)lb * kWaves + wave; tile < ntiles; tile += (long long)nb * kWaves) {
    asm volatile("" ::: "memory");  // keep the tile-invariant LDS reads inside the persistent loop (mm_policy_mfma.h)
    const long long local = tile * 32 + j;
    const bool live = local < ng;
    const long long ag = g0 + local;  // the global agent index: the row of obs / logp / actions and the sampler's key
    f32x16 x[1];                      // B operand of layer 1: x[agent j][k(s, h)]
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const int k = frag_row(s, h);
      x[0][s] = (live && k < n_s) ? obs[ag * n_s + k] : 0.0f;
    }
    f32x16 h1[4], h2[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; r++) acc[r] = sB1[32 * m + frag_row(r, h)];
      h1[m] = relu(fc2_tile<1>(sW1[m], x, lane, acc));
    }
#pragma unroll
    for (int m = 0; m < 4; m++) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; r++) acc[r] = sB2[32 * m + frag_row(r, h)];
      h2[m] = relu(fc2_tile<4>(sW2[m], h1, lane, acc));
    }
    // ---- layer 3 + log-softmax + sample
    float logit[8];
#pragma unroll
    for (int o = 0; o < 8; o++) {
      const float p = head_dot(h2, sW3[o], h, o < n_a);
      logit[o] = o < n_a ? p + sB3[o] : -INFINITY;
    }
    const float mx = max8(logit);
    float se = 0.0f;
#pragma unroll
    for (int o = 0; o < 8; o++) se += exp_shifted(logit[o], mx, o < n_a);
    const float lg = logf(se);  // (logit - mx) - log(sum), as policy_kernel: the normaliser is not rounded at ulp(mx)
    if (live && h == 0) {
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

__global__ void counter_bump_kernel(uint64_t *counter) { *counter += 1; }

static bool groups_ok(int32_t K, const int64_t *group_start) {
  if (!group_start || K < 1 || K > MM_BANK_MAX_GROUPS || group_start[0] != 0) return false;
  for (int k = 0; k < K; k++)
    if (group_start[k + 1] < group_start[k]) return false;
  return true;
}

// the block prefix of a checked group table (file header: the grid split)
static void bank_grid(int32_t K, const int64_t *group_start, int32_t *block_start) {
  long long tiles[MM_BANK_MAX_GROUPS], cap[MM_BANK_MAX_GROUPS], blocks[MM_BANK_MAX_GROUPS], total = 0, cap_sum = 0;
  for (int k = 0; k < K; k++) {
    tiles[k] = (group_start[k + 1] - group_start[k] + MM_BANK_TILE - 1) / MM_BANK_TILE;
    cap[k] = (tiles[k] + kWaves - 1) / kWaves;  // a workgroup past this one would have no tile
    total += tiles[k];
    cap_sum += cap[k];
  }
  if (cap_sum <= MM_BANK_MAX_GRID) {
    for (int k = 0; k < K; k++) blocks[k] = cap[k];  // every wave at most one tile
  } else {
    long long used = 0;
    for (int k = 0; k < K; k++) {
      long long share = (long long)((__int128)MM_BANK_MAX_GRID * tiles[k] / total);
      if (share > cap[k]) share = cap[k];
      blocks[k] = tiles[k] > 0 && share < 1 ? 1 : share;
      used += blocks[k];
    }
    for (; used < MM_BANK_MAX_GRID; used++) {  // the rounding's rest: to the group with the most tiles per workgroup
      int best = -1;
      for (int k = 0; k < K; k++) {
        if (blocks[k] >= cap[k]) continue;
        if (best < 0 || (__int128)tiles[k] * blocks[best] > (__int128)tiles[best] * blocks[k]) best = k;
      }
      if (best < 0) break;
      blocks[best]++;
    }
  }
  block_start[0] = 0;
  for (int k = 0; k < K; k++) block_start[k + 1] = block_start[k] + (int32_t)blocks[k];
}

}  // namespace bank
}  // namespace mm

extern "C" int32_t mm_policy_bank_grid(int32_t K, const int64_t *group_start, int32_t *block_start) {
  if (!block_start || !mm::bank::groups_ok(K, group_start)) return MM_ERR_INVALID_ARG;
  mm::bank::bank_grid(K, group_start, block_start);
  return MM_OK;
}

extern "C" int32_t mm_policy_bank_act(const float *obs, int64_t n, int32_t n_s, const MMMlpParams *bank, int32_t K,
                                      const int64_t *group_start, int32_t hidden, int32_t n_a, uint64_t seed, uint64_t *counter,
                                      int32_t *actions, float *logp, MMStream stream) {
  using namespace mm::bank;
  if (!obs || !mm::mfma::complete(bank) || !counter || !actions) return MM_ERR_INVALID_ARG;
  if (n < 0 || n_s < 1 || n_s > 32 || hidden != kHidden || n_a < 1 || n_a > 8) return MM_ERR_INVALID_ARG;
  if (!groups_ok(K, group_start) || group_start[K] != n) return MM_ERR_INVALID_ARG;
  if (n == 0) return MM_OK;
  Args a;
  a.w = *bank;
  bank_grid(K, group_start, a.block_start);
  for (int k = 0; k <= MM_BANK_MAX_GROUPS; k++) {
    a.group_start[k] = group_start[k < K ? k : K];
    if (k > K) a.block_start[k] = a.block_start[K];
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(policy_bank_kernel, dim3((unsigned)a.block_start[K]), dim3(kThreads), 0, s, obs, (int)n_s, a, (int)n_a, seed,
                     (const uint64_t *)counter, actions, logp);
  hipLaunchKernelGGL(counter_bump_kernel, dim3(1), dim3(1), 0, s, counter);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
