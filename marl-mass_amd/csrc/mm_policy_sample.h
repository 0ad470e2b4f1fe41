// mm_policy_sample.h -- kernel A of the hidden-128 separate actor / critic, once: what mm_policy_train.hip runs on one network's
// batch and mm_policy_bank_train.hip on the K members' column groups.  Both networks are "n_s -> 128 -> 128 -> head", so the one
// text serves them (kCritic) and, without the backward, the forward-only evaluations (!kTrain).
//
// The body IS the kernel template: shared this way both files' kernels are the recorded instructions, as a force-inlined function
// they are not (mm_policy_mfma.h, "How the helpers are cut").  The kernel's arguments are the file's own by-value blocks, and a
// policy type `Where`, built from them, says where a workgroup's network, samples and scratch rows live -- nothing else differs:
//   p                     the block that carries obs, actions, valid, returns, old_logp, n_s, n_a, clip_param, huber, the scratch
//                         rows s_h1 .. s_xs and out0 / out1 under these names
//   net(n_s, k2, n_out)   the network's six tensors;  frag(), lossp(): its W2^T fragments and the loss partial of its tile 0
//   n()                   its samples; a wave walks their 32-sample tiles first_tile(wave), + tile_stride(), ...
//   count()               B, the valid samples behind the 1 / B factors;  adv_sums(): its S+ / S- pair;  ref_form()
//   sample(i, in_range)   local sample i -> the batch's sample index (inputs, out0 / out1);  row(i): its scratch row
//   advantage(ag)         the per-sample form's advantage of batch sample ag
//
//   kernel A  per sample: fc1 (K = n_s padded to 32: 16 k-steps x 4 tiles), fc2 (K = 128: 64 k-steps x 4 tiles), the head on
//             the VALU (<= 8 rows), then the loss terms and dlogit / dvalue; dz2 = W3^T dhead . [h2 > 0] on the VALU;
//             dz1 = (W2[:, :128]^T dz2) . [h1 > 0] as a second 128 x 128 MFMA contraction whose A operand comes from the
//             fragment array `prep` wrote (global, L2 resident: reading transposed fragments out of the one staged LDS copy
//             would put the 64 lanes of a read on 8 banks -- the trap recorded at dz1_tile in mm_policy_mfma.h).
//             The critic's fc2 has K = 128 + n_a with a one-hot block: in the forward that block is a column gather,
//             z2 = b2 + W2[:, 128 + a_j] + W2[:, :128] h1, added where the accumulator is initialised, out of an [8][128]
//             LDS table (rows padded to 136 floats: lanes with different actions land on different banks); in the backward
//             dW2[:, 128 + a] = sum_j dz2_j [a_j = a] is a fifth column tile of kernel B whose B operand is the one-hot row
//             rebuilt from the action kept in the sample's head row.  No gradient flows into the one-hot input.
//             Stores h1, dz1, h2, dz2 (128 each), dhead (16: the actor's dlogit 0..7 | the critic's dvalue in column 0 and
//             the clamped action, as a float, in column 15) and x (32: the observation, zeros past n_s) per sample in
//             [sample][feature] order, gradient rows of masked / out-of-range samples as exact zeros, and one loss partial
//             per 32 samples in fp64.
#ifndef MM_POLICY_SAMPLE_H
#define MM_POLICY_SAMPLE_H
#include "mm_policy_mfma.h"

namespace mm {
namespace mfma {

constexpr int kOhPitch = 136;   // row pitch of the one-hot column table in LDS
constexpr int kThreadsA = 512;  // 8 waves = 2 per SIMD

template <bool kCritic, bool kTrain, class Where, class... Args>
__global__ __launch_bounds__(kThreadsA) void mlp_sample_kernel(const Args... a) {
  __shared__ float4 sW1[4][4][64];   // [out tile][k-step / 4][lane]: 16 KB
  __shared__ float4 sW2[4][16][64];  // [out tile][k-step / 4][lane]: 64 KB
  __shared__ __attribute__((aligned(16))) float sWh[8][kHidden];  // head rows (zero past the head's width): 4 KB
  __shared__ __attribute__((aligned(16))) float sOh[kCritic ? 8 : 1][kOhPitch];  // critic: fc2's one-hot columns, [action][feature]
  __shared__ __attribute__((aligned(16))) float sB1[kHidden], sB2[kHidden];
  __shared__ float sBh[8];
  const Where wh(a...);
  const auto &p = wh.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int n_s = p.n_s, n_a = p.n_a;
  const int k2 = kCritic ? kHidden + n_a : kHidden;  // fc2's row length
  const int n_out = kCritic ? 1 : n_a;
  const MMMlpParams w = wh.net(n_s, k2, n_out);
  const float *__restrict__ W1 = w.W1, *__restrict__ W2 = w.W2, *__restrict__ W3 = w.W3;
  for (int t = tid; t < 4 * 4 * 64; t += kThreadsA) {
    const int l = t & 63, q = (t >> 6) & 3, m = t >> 8;
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = 2 * (4 * q + u) + (l >> 5);
      v[u] = k < n_s ? W1[(32 * m + (l & 31)) * n_s + k] : 0.0f;
    }
    sW1[m][q][l] = make_float4(v[0], v[1], v[2], v[3]);
  }
  for (int t = tid; t < 4 * 16 * 64; t += kThreadsA) {
    const int l = t & 63, q = (t >> 6) & 15, m = t >> 10;
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int s = 4 * q + u;
      v[u] = W2[(32 * m + (l & 31)) * k2 + 32 * (s >> 4) + frag_row(s & 15, l >> 5)];
    }
    sW2[m][q][l] = make_float4(v[0], v[1], v[2], v[3]);
  }
  for (int t = tid; t < 8 * kHidden; t += kThreadsA) {
    const int o = t / kHidden, c = t % kHidden;
    sWh[o][c] = o < n_out ? W3[o * kHidden + c] : 0.0f;
    if constexpr (kCritic) sOh[o][c] = o < n_a ? W2[c * k2 + kHidden + o] : 0.0f;
  }
  if (tid < kHidden) {
    sB1[tid] = w.b1[tid];
    sB2[tid] = w.b2[tid];
  }
  if (tid < 8) sBh[tid] = tid < n_out ? w.b3[tid] : 0.0f;
  __syncthreads();
  int nb = 0;
  if (kTrain) nb = wh.count();
  const float inv_b = nb > 0 ? 1.0f / (float)nb : 0.0f;
  const bool ref_form = wh.ref_form();
  const double sp_d = (kTrain && !kCritic && ref_form) ? (double)wh.adv_sums()[0] : 0.0;
  const double sn_d = (kTrain && !kCritic && ref_form) ? (double)wh.adv_sums()[1] : 0.0;
  const RefWeights ref_w = ref_weights(sp_d, sn_d, nb);
  const float lo = 1.0f - p.clip_param, hi = 1.0f + p.clip_param;
  const long long n = wh.n(), ntiles = (n + 31) / 32;
  const float4 *const frag = wh.frag();
  double *const lossp = wh.lossp();
  for (long long tile = wh.first_tile(wave); tile < ntiles; tile += wh.tile_stride()) {
    asm volatile("" ::: "memory");  // keep the tile-invariant LDS reads inside the persistent loop (mm_policy_mfma.h)
    const long long local = tile * 32 + j;
    const bool inr = local < n;
    const long long ag = wh.sample(local, inr);  // the batch's sample index
    const long long sr = wh.row(local);          // the scratch row
    bool live = inr;
    if (live && p.valid) live = p.valid[ag] != 0;
    const float *row = p.obs + (live ? ag : 0) * p.obs_stride;
    int act = live ? p.actions[ag * p.act_stride] : 0;
    act = act < 0 ? 0 : (act > n_a - 1 ? n_a - 1 : act);
    float x[16];
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const int k = 2 * s + h;
      x[s] = (live && k < n_s) ? row[k] : 0.0f;
    }
    if (kTrain) {  // x row of the scratch: columns 16 h .. 16 h + 15, zeros past n_s and for a masked sample
      float4 *dst = reinterpret_cast<float4 *>(p.s_xs + sr * kXs + 16 * h);
#pragma unroll
      for (int g = 0; g < 4; g++) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int c = 16 * h + 4 * g + u;
          v[u] = (live && c < n_s) ? row[c] : 0.0f;
        }
        dst[g] = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    f32x16 h1[4], h2[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      f32x16 acc;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float4 b = *reinterpret_cast<const float4 *>(&sB1[32 * m + 8 * g + 4 * h]);
        acc[4 * g] = b.x; acc[4 * g + 1] = b.y; acc[4 * g + 2] = b.z; acc[4 * g + 3] = b.w;
      }
#pragma unroll
      for (int q = 0; q < 4; q++) acc = mfma4(sW1[m][q][lane], x[4 * q + 0], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3], acc);
      h1[m] = relu(acc);
      if (kTrain) store_tile(p.s_h1 + sr * kHidden + 32 * m + 4 * h, h1[m]);
    }
#pragma unroll
    for (int m = 0; m < 4; m++) {
      f32x16 acc;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        float4 b = *reinterpret_cast<const float4 *>(&sB2[32 * m + 8 * g + 4 * h]);
        if constexpr (kCritic) {  // the one-hot block of fc2: column 128 + act
          const float4 o = *reinterpret_cast<const float4 *>(&sOh[act][32 * m + 8 * g + 4 * h]);
          b.x += o.x; b.y += o.y; b.z += o.z; b.w += o.w;
        }
        acc[4 * g] = b.x; acc[4 * g + 1] = b.y; acc[4 * g + 2] = b.z; acc[4 * g + 3] = b.w;
      }
      h2[m] = relu(fc2_tile<4>(sW2[m], h1, lane, acc));
      if (kTrain) store_tile(p.s_h2 + sr * kHidden + 32 * m + 4 * h, h2[m]);
    }
    // ---- head, the objective's per-sample terms, dhead (both lane halves compute the same numbers)
    float dhead[8];
    double t_loss = 0.0;
    if (kCritic) {
      float v = 0.0f;
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) v = fmaf(h2[m][r], sWh[0][32 * m + frag_row(r, h)], v);
      v = v + __shfl_xor(v, 32, 64) + sBh[0];
      if (h == 0 && inr && p.out0) p.out0[ag] = live ? v : 0.0f;
      if (!kTrain) continue;
      const float ret = live ? p.returns[ag * p.ret_stride] : 0.0f;
      const float d = v - ret;
      float t_critic, dv;
      critic_term(d, p.huber, t_critic, dv);
      t_loss = (double)t_critic;
      dhead[0] = live ? dv * inv_b : 0.0f;
#pragma unroll
      for (int o = 1; o < 8; o++) dhead[o] = 0.0f;
    } else {
      float logit[8];
#pragma unroll
      for (int o = 0; o < 8; o++) {
        const float s = head_dot(h2, sWh[o], h, o < n_a);
        logit[o] = o < n_a ? s + sBh[o] : -INFINITY;
      }
      const float mx = max8(logit);
      float se = 0.0f;
#pragma unroll
      for (int o = 0; o < 8; o++) se += exp_shifted(logit[o], mx, o < n_a);
      const float lse = mx + logf(se);
      const float lp_a = logp_taken(logit, lse, act);
      if (!kTrain) {
        if (h == 0 && inr && p.out0) p.out0[ag] = live ? lp_a : 0.0f;
        continue;
      }
      const float olp = live ? p.old_logp[ag] : 0.0f;
      const float r = expf(lp_a - olp);
      const float c = fminf(fmaxf(r, lo), hi);
      float wsel;
      if (ref_form) ppo_clip_ref(sp_d, sn_d, ref_w, lo, hi, r, c, t_loss, wsel);
      else ppo_clip_flat(live ? wh.advantage(ag) : 0.0f, lo, hi, r, c, t_loss, wsel);
      const float g_lp = live ? -inv_b * wsel * r : 0.0f;  // d loss / d logp_taken
#pragma unroll
      for (int o = 0; o < 8; o++) dhead[o] = (o < n_a) ? dlogit(g_lp, logit[o], lse, o == act) : 0.0f;
      if (h == 0 && inr) {
        if (p.out0) p.out0[ag] = live ? lp_a : 0.0f;
        if (p.out1) p.out1[ag] = live ? r : 0.0f;
      }
    }
    {
      float4 *dst = reinterpret_cast<float4 *>(p.s_dh + sr * kDh + 8 * h);
      if (h == 0) {
        dst[0] = make_float4(dhead[0], dhead[1], dhead[2], dhead[3]);
        dst[1] = make_float4(dhead[4], dhead[5], dhead[6], dhead[7]);
      } else {
        dst[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        dst[1] = make_float4(0.0f, 0.0f, 0.0f, kCritic ? (float)act : 0.0f);  // column kActCol
      }
    }
    // loss partial of this tile: lanes of half 0, fixed butterfly
    {
      double pl = (live && h == 0) ? t_loss : 0.0;
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) pl += __shfl_xor(pl, o, 64);
      if (lane == 0) lossp[tile] = pl;
    }
    // ---- dz2 = (W3^T dhead) . [h2 > 0], in accumulator form (reuses h2's registers)
#pragma unroll
    for (int m = 0; m < 4; m++) {
#pragma unroll
      for (int g = 0; g < 4; g++) {
        // the lane's features 32 m + 8 g + 4 h .. + 3 are contiguous in a head row: one ds_read_b128 per row.  Rows past
        // the head's width are zero in sWh and their dhead is zero, so all rows are summed without a branch.
        const int f = 32 * m + 8 * g + 4 * h;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
        for (int o = 0; o < (kCritic ? 1 : 8); o++) {
          const float4 wa = *reinterpret_cast<const float4 *>(&sWh[o][f]);
          s0 = fmaf(dhead[o], wa.x, s0);
          s1 = fmaf(dhead[o], wa.y, s1);
          s2 = fmaf(dhead[o], wa.z, s2);
          s3 = fmaf(dhead[o], wa.w, s3);
        }
        h2[m][4 * g + 0] = h2[m][4 * g + 0] > 0.0f ? s0 : 0.0f;
        h2[m][4 * g + 1] = h2[m][4 * g + 1] > 0.0f ? s1 : 0.0f;
        h2[m][4 * g + 2] = h2[m][4 * g + 2] > 0.0f ? s2 : 0.0f;
        h2[m][4 * g + 3] = h2[m][4 * g + 3] > 0.0f ? s3 : 0.0f;
      }
      store_tile(p.s_dz2 + sr * kHidden + 32 * m + 4 * h, h2[m]);
    }
    // ---- dz1 = (W2[:, :128]^T dz2) . [h1 > 0]: 4 output tiles x 64 k-steps, A fragments from global memory
    const unsigned vlane = opaque_lane(lane);
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {
      const f32x16 acc = dz1_tile(frag, mt, vlane, h2);
#pragma unroll
      for (int g = 0; g < 4; g++) {
        float4 *dst = reinterpret_cast<float4 *>(p.s_dz1 + sr * kHidden + 32 * mt + 4 * h);
        dst[2 * g] = make_float4(h1[mt][4 * g] > 0.0f ? acc[4 * g] : 0.0f, h1[mt][4 * g + 1] > 0.0f ? acc[4 * g + 1] : 0.0f,
                                 h1[mt][4 * g + 2] > 0.0f ? acc[4 * g + 2] : 0.0f, h1[mt][4 * g + 3] > 0.0f ? acc[4 * g + 3] : 0.0f);
      }
    }
  }
}

}  // namespace mfma
}  // namespace mm
#endif
