// mm_policy_gi_sample.h -- kernel A of MAPPO_GI's shared actor-critic at hidden 128, once: what mm_policy_gi_train.hip runs on one
// network's batch (and, through launch_sample, the chunked and rank-sharded passes) and mm_policy_gi_bank_train.hip on the K
// members' column groups, and, without the backward (!kTrain), the bank's forward-only evaluation.
//
// The body is a force-inlined function template that a __global__ of each file calls: policy_gi_train_sample_kernel keeps its
// name and its argument list (the pass loops launch it by that signature), so the text cannot be the kernel template itself as
// in mm_policy_sample.h.  A policy type `Where`, built by the calling kernel from its own arguments, says where a workgroup's
// network, samples and scratch rows live -- nothing else differs:
//   p                     the block that carries obs, obs_stride, actions, act_stride, returns, ret_stride, old_logp, valid, n_a,
//                         clip_param, huber, the scratch rows s_h1 .. s_xs and logp_out / value_out / ratio_out under these names
//   net()                 the network's twelve tensors;  frag(), lossp(): its W2^T fragments and the loss partials of its tile 0
//   n()                   its samples; a wave walks their 32-sample tiles first_tile(wave), + tile_stride(), ...
//   count()               B, the valid samples behind the 1 / B factors;  adv_sums(): its S+ / S- pair;  ref_form()
//   sample(i, in_range)   local sample i -> the batch's sample index (inputs, outputs);  row(i): its scratch row
//
//   kernel A  per sample: forward (the split gather of layer 1, fc2 160 -> 128 on f32 MFMA), heads, log-softmax, ratio, the loss
//             terms, dlogit / dvalue (VALU tail); dz2 = (Wa^T dlogit + Wc^T dvalue) . [h2 > 0] on the VALU (<= 9 rows, 64
//             features per lane); dz1 = (W2^T dz2) . [h1 > 0] as a second 160 x 128 MFMA contraction (5 tiles x 64 k-steps; dz2
//             in accumulator form is its B operand as h1 is the forward's), its A operand 80 float4 loads per lane and tile
//             from the 80 KB fragment array (global, L2 resident: dz1_tile in mm_policy_mfma.h says why).
//             Stores h1, dz1 (160), h2, dz2 (128), dhead (16: dlogit 0..7, dvalue, zeros) and x (32: columns 0..24 of the
//             observation, zeros) per sample in [sample][feature] order, rows of masked / out-of-range samples as exact
//             zeros in every gradient row, and one (actor, critic) loss partial per 32 samples in fp64.
//   !kTrain   the forward alone, with the outputs formed as policy_gi_kernel forms them (mm_policy_gi.hip): the taken action's
//             log-probability is (logit - max) - log(sum), the normaliser not rounded at ulp(max), and the value is the row's
//             -- bit for bit what mm_policy_gi_act writes for that observation.  Nothing of the scratch is touched.
#ifndef MM_POLICY_GI_SAMPLE_H
#define MM_POLICY_GI_SAMPLE_H
#include "mm_policy_mfma.h"

namespace mm {
namespace mfma {

constexpr int kGiCat = 160;               // hidden / 4 + hidden / 2 + hidden / 2
constexpr int kGiL1Steps = 3 + 4 * 5;     // A fragments of layer 1: fc11 3 k-steps, 4 tiles of fc12 / fc13 x 5
constexpr int kGiThreadsA = 512;          // 8 waves = 2 per SIMD, as policy_gi_kernel

template <bool kTrain, class Where>
MM_DEV void gi_sample_body(const Where &wh) {
  constexpr int kCat = kGiCat, kL1Steps = kGiL1Steps, kThreadsA = kGiThreadsA;
  __shared__ float sW1[kL1Steps][64];   // [fragment][lane]: 5.75 KB
  __shared__ float4 sW2[4][20][64];     // [out tile][k-step / 4][lane]: 80 KB
  __shared__ __attribute__((aligned(16))) float sWh[9][kHidden];  // actor_linear rows 0..7 (zero past n_a), critic_linear row 8: 4.5 KB
  __shared__ float sB1[kCat], sB2[kHidden], sBh[9];
  const auto &p = wh.p;
  const MMGiParams w = wh.net();
  const int n_a = p.n_a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  for (int t = tid; t < kL1Steps * 64; t += kThreadsA) {
    const int l = t & 63, q = t >> 6;
    int m, s;
    l1_step(q, m, s);
    const int k = 2 * s + (l >> 5);
    float v;
    if (m == 0) v = k < 5 ? w.W11[(l & 31) * 5 + k] : 0.0f;
    else if (m <= 2) v = w.W12[(32 * (m - 1) + (l & 31)) * 10 + k];
    else v = w.W13[(32 * (m - 3) + (l & 31)) * 10 + k];
    sW1[q][l] = v;
  }
  stage_w2<20, kThreadsA>(sW2, w.W2, kCat);
  for (int t = tid; t < 9 * kHidden; t += kThreadsA) {
    const int o = t / kHidden, c = t % kHidden;
    sWh[o][c] = o == 8 ? w.Wc[c] : (o < n_a ? w.Wa[o * kHidden + c] : 0.0f);
  }
  if (tid < 32) sB1[tid] = w.b11[tid];
  else if (tid < 96) sB1[tid] = w.b12[tid - 32];
  else if (tid < kCat) sB1[tid] = w.b13[tid - 96];
  if (tid < kHidden) sB2[tid] = w.b2[tid];
  if (tid < 9) sBh[tid] = tid == 8 ? w.bc[0] : (tid < n_a ? w.ba[tid] : 0.0f);
  __syncthreads();
  int nb = 0;
  if (kTrain) nb = wh.count();
  const float inv_b = nb > 0 ? 1.0f / (float)nb : 0.0f;
  const bool ref_form = kTrain && wh.ref_form();
  const double sp_d = ref_form ? (double)wh.adv_sums()[0] : 0.0, sn_d = ref_form ? (double)wh.adv_sums()[1] : 0.0;
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
    // x row of the scratch: columns 16 h .. 16 h + 15 (0..24 kept), zeros for a masked sample
    if (kTrain) {
      float4 *dst = reinterpret_cast<float4 *>(p.s_xs + sr * kXs + 16 * h);
#pragma unroll
      for (int g = 0; g < 4; g++) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int c = 16 * h + 4 * g + u;
          v[u] = (live && c < 25) ? row[c] : 0.0f;
        }
        dst[g] = make_float4(v[0], v[1], v[2], v[3]);
      }
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
      if (kTrain) store_tile(p.s_h1 + sr * kCat + 32 * m + 4 * h, h1[m]);
    }
#pragma unroll
    for (int m = 0; m < 4; m++) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; r++) acc[r] = sB2[32 * m + frag_row(r, h)];
      h2[m] = relu(fc2_tile<5>(sW2[m], h1, lane, acc));
      if (kTrain) store_tile(p.s_h2 + sr * kHidden + 32 * m + 4 * h, h2[m]);
    }
    // ---- heads
    float logit[8];
#pragma unroll
    for (int o = 0; o < 8; o++) {
      const float pd = head_dot(h2, sWh[o], h, o < n_a);
      logit[o] = o < n_a ? pd + sBh[o] : -INFINITY;
    }
    float v = 0.0f;
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
      for (int r = 0; r < 16; r++) v = fmaf(h2[m][r], sWh[8][32 * m + frag_row(r, h)], v);
    v = v + __shfl_xor(v, 32, 64) + sBh[8];
    const float mx = max8(logit);
    float se = 0.0f;
#pragma unroll
    for (int o = 0; o < 8; o++) se += exp_shifted(logit[o], mx, o < n_a);
    if (!kTrain) {  // the outputs as policy_gi_kernel writes them
      int act = live ? p.actions[ag * p.act_stride] : 0;
      act = act < 0 ? 0 : (act > n_a - 1 ? n_a - 1 : act);
      const float lg = logf(se);
      float lp = 0.0f;
#pragma unroll
      for (int o = 0; o < 8; o++) lp = (o == act) ? (logit[o] - mx) - lg : lp;
      if (h == 0 && inr) {
        if (p.logp_out) p.logp_out[ag] = live ? lp : 0.0f;
        if (p.value_out) p.value_out[ag] = live ? v : 0.0f;
      }
      continue;
    }
    const float lse = mx + logf(se);
    // ---- the objective's per-sample terms (both lane halves compute the same numbers)
    int act = live ? p.actions[ag * p.act_stride] : 0;
    act = act < 0 ? 0 : (act > n_a - 1 ? n_a - 1 : act);
    const float ret = live ? p.returns[ag * p.ret_stride] : 0.0f;
    const float olp = live ? p.old_logp[ag] : 0.0f;
    const float lp_a = logp_taken(logit, lse, act);
    const float r = expf(lp_a - olp);
    const float adv = ret - v;
    const float c = fminf(fmaxf(r, lo), hi);
    double t_actor;
    float wsel;
    if (ref_form) ppo_clip_ref(sp_d, sn_d, ref_w, lo, hi, r, c, t_actor, wsel);
    else ppo_clip_flat(adv, lo, hi, r, c, t_actor, wsel);
    const float dldr = -inv_b * wsel;
    const float d = v - ret;
    float t_critic, dv;
    critic_term(d, p.huber, t_critic, dv);
    dv = live ? dv * inv_b : 0.0f;
    float dlogit[8];
    const float g_lp = live ? dldr * r : 0.0f;  // d loss / d logp_taken
#pragma unroll
    for (int o = 0; o < 8; o++) dlogit[o] = (o < n_a) ? mfma::dlogit(g_lp, logit[o], lse, o == act) : 0.0f;
    {
      float4 *dst = reinterpret_cast<float4 *>(p.s_dh + sr * kDh + 8 * h);
      if (h == 0) {
        dst[0] = make_float4(dlogit[0], dlogit[1], dlogit[2], dlogit[3]);
        dst[1] = make_float4(dlogit[4], dlogit[5], dlogit[6], dlogit[7]);
      } else {
        dst[0] = make_float4(dv, 0.0f, 0.0f, 0.0f);
        dst[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
    }
    if (h == 0 && inr) {
      if (p.logp_out) p.logp_out[ag] = live ? lp_a : 0.0f;
      if (p.value_out) p.value_out[ag] = live ? v : 0.0f;
      if (p.ratio_out) p.ratio_out[ag] = live ? r : 0.0f;
    }
    // loss partial of this tile: lanes of half 0, fixed butterfly
    {
      double pa = (live && h == 0) ? t_actor : 0.0, pc = (live && h == 0) ? (double)t_critic : 0.0;
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) {
        pa += __shfl_xor(pa, o, 64);
        pc += __shfl_xor(pc, o, 64);
      }
      if (lane == 0) {
        lossp[2 * tile] = pa;
        lossp[2 * tile + 1] = pc;
      }
    }
    // ---- dz2 = (Wa^T dlogit + Wc^T dvalue) . [h2 > 0], in accumulator form (reuses h2's registers)
#pragma unroll
    for (int m = 0; m < 4; m++) {
#pragma unroll
      for (int g = 0; g < 4; g++) {
        // the lane's features 32 m + 8 g + 4 h .. + 3 are contiguous in a head row: one ds_read_b128 per row.  Rows past
        // n_a are zero in sWh and their dlogit is zero, so all 9 rows are summed without a branch.
        const int f = 32 * m + 8 * g + 4 * h;
        const float4 wc = *reinterpret_cast<const float4 *>(&sWh[8][f]);
        float s0 = dv * wc.x, s1 = dv * wc.y, s2 = dv * wc.z, s3 = dv * wc.w;
#pragma unroll
        for (int o = 0; o < 8; o++) {
          const float4 wa = *reinterpret_cast<const float4 *>(&sWh[o][f]);
          s0 = fmaf(dlogit[o], wa.x, s0);
          s1 = fmaf(dlogit[o], wa.y, s1);
          s2 = fmaf(dlogit[o], wa.z, s2);
          s3 = fmaf(dlogit[o], wa.w, s3);
        }
        h2[m][4 * g + 0] = h2[m][4 * g + 0] > 0.0f ? s0 : 0.0f;
        h2[m][4 * g + 1] = h2[m][4 * g + 1] > 0.0f ? s1 : 0.0f;
        h2[m][4 * g + 2] = h2[m][4 * g + 2] > 0.0f ? s2 : 0.0f;
        h2[m][4 * g + 3] = h2[m][4 * g + 3] > 0.0f ? s3 : 0.0f;
      }
      store_tile(p.s_dz2 + sr * kHidden + 32 * m + 4 * h, h2[m]);
    }
    // ---- dz1 = (W2^T dz2) . [h1 > 0]: 5 output tiles x 64 k-steps, A fragments from global memory
    const unsigned vlane = opaque_lane(lane);
#pragma unroll
    for (int mt = 0; mt < 5; mt++) {
      const f32x16 acc = dz1_tile(frag, mt, vlane, h2);
      // the ReLU mask of layer 1 is read back from this lane's own h1 stores (L2 / L1 hot) instead of holding h1's 80
      // registers across the heads and the second contraction
      const float4 *msk = reinterpret_cast<const float4 *>(p.s_h1 + sr * kCat + 32 * mt + 4 * h);
      float4 *dst = reinterpret_cast<float4 *>(p.s_dz1 + sr * kCat + 32 * mt + 4 * h);
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float4 a = msk[2 * g];
        dst[2 * g] = make_float4(a.x > 0.0f ? acc[4 * g] : 0.0f, a.y > 0.0f ? acc[4 * g + 1] : 0.0f,
                                 a.z > 0.0f ? acc[4 * g + 2] : 0.0f, a.w > 0.0f ? acc[4 * g + 3] : 0.0f);
      }
    }
  }
}

}  // namespace mfma
}  // namespace mm
#endif
