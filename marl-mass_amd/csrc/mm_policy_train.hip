// mm_policy_train.hip -- loss and parameter gradient of MAPPO's separate actor and critic (include/mm_policy_train.h), and the
// forward-only mm_policy_eval.
//
// The shape is mm_policy_gi_train.hip's, in the layout and from the pieces of mm_policy_mfma.h.  Both networks are
// "n_s -> 128 -> 128 -> head", so ONE kernel template serves them (kCritic) and, without the backward, mm_policy_eval (!kTrain).
//
//   prep      W2[:, :128]^T of each given network in MFMA A-fragment order into the scratch (64 KB each), and B = the number
//             of valid samples.
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
//   kernel B  contractions over the sample dimension, the sample index as the MFMA k dimension, both operands coalesced row
//             reads of the scratch: dW2 = dz2^T [h1 | one_hot] (4 x 4 or 4 x 5 tiles), dW3 = dhead^T h2 (4 tiles), dW1 =
//             dz1^T x (4 tiles), bias sums on the VALU from the A operands.  5 waves per workgroup: wave w < 4 owns output
//             rows 32 w .. 32 w + 31 of dW2 and columns of the head tile, wave 4 the first layer.  Each workgroup contracts one
//             contiguous slice of samples and writes one partial block.
//   kernel C  every parameter's gradient = the partial blocks summed in workgroup order (fp64 running sum), written in
//             torch layout; the loss partials folded by one workgroup in a fixed tree.
// The actor's three kernels run first, then the critic's over the same scratch (stream order).
#include "mm_policy_chunked.h"  // PassArgs and the launch helpers' declarations; mm_policy_mfma.h and the public header

namespace mm {
namespace pt {

using namespace mfma;
constexpr int kCat = kW2Pitch;  // row pitch of the dW2 partial: 128 + the one-hot tile
constexpr int kOhPitch = 136;   // row pitch of the one-hot column table in LDS
constexpr int kThreadsA = 512;  // 8 waves = 2 per SIMD
constexpr int kThreadsB = 320;  // 5 waves

constexpr long long kFrag = 4 * 4 * 4 * 64 * 4;  // W2^T fragments of one network, in floats: [out tile 4][k chunk 4][group 4][lane 64] float4
typedef PartialBlock<4> Part;                    // the partial block of one kernel-B workgroup: 26 896 floats

static Layout layout(long long n) { return scratch_layout(n, 2 * kFrag, kHidden, 1, Part::kSize); }  // (the actor's fragments, then the critic's)

// ---- prep: W2[:, :128]^T fragments of the given networks + the count of valid samples (integer atomics: order-independent)
__global__ __launch_bounds__(256) void policy_train_prep_kernel(const float *__restrict__ W2a, const float *__restrict__ W2c, int k2c,
                                                                float4 *__restrict__ frag, const uint8_t *__restrict__ valid,
                                                                long long n, int *__restrict__ count) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < 2 * 4096) {
    const bool crit = t >= 4096;
    const float *W2 = crit ? W2c : W2a;
    const int k2 = crit ? k2c : kHidden;
    if (W2) frag[t] = w2t_fragment(W2, k2, t & 4095);
  }
  if (!count) return;
  count_valid(valid, n, t, count);
}

struct SampleArgs {
  const float *obs;
  long long obs_stride, n;
  int n_s;
  const int32_t *actions;
  long long act_stride;
  const float *returns;
  long long ret_stride;
  const float *old_logp;
  const uint8_t *valid;
  MMMlpParams w;
  int n_a;
  float clip_param;
  int huber;
  const float *adv_sums, *advantages;
  const int *count;
  const float4 *frag;
  float *s_h1, *s_dz1, *s_h2, *s_dz2, *s_dh, *s_xs;
  double *lossp;
  float *out0, *out1;  // actor: logp_taken, ratio; critic: value, unused
};

// ---- kernel A
template <bool kCritic, bool kTrain>
__global__ __launch_bounds__(kThreadsA) void policy_train_sample_kernel(const SampleArgs p) {
  __shared__ float4 sW1[4][4][64];   // [out tile][k-step / 4][lane]: 16 KB
  __shared__ float4 sW2[4][16][64];  // [out tile][k-step / 4][lane]: 64 KB
  __shared__ __attribute__((aligned(16))) float sWh[8][kHidden];  // head rows (zero past the head's width): 4 KB
  __shared__ __attribute__((aligned(16))) float sOh[kCritic ? 8 : 1][kOhPitch];  // critic: fc2's one-hot columns, [action][feature]
  __shared__ __attribute__((aligned(16))) float sB1[kHidden], sB2[kHidden];
  __shared__ float sBh[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int n_s = p.n_s, n_a = p.n_a;
  const int k2 = kCritic ? kHidden + n_a : kHidden;  // fc2's row length
  const int n_out = kCritic ? 1 : n_a;
  for (int t = tid; t < 4 * 4 * 64; t += kThreadsA) {
    const int l = t & 63, q = (t >> 6) & 3, m = t >> 8;
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = 2 * (4 * q + u) + (l >> 5);
      v[u] = k < n_s ? p.w.W1[(32 * m + (l & 31)) * n_s + k] : 0.0f;
    }
    sW1[m][q][l] = make_float4(v[0], v[1], v[2], v[3]);
  }
  for (int t = tid; t < 4 * 16 * 64; t += kThreadsA) {
    const int l = t & 63, q = (t >> 6) & 15, m = t >> 10;
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int s = 4 * q + u;
      v[u] = p.w.W2[(32 * m + (l & 31)) * k2 + 32 * (s >> 4) + frag_row(s & 15, l >> 5)];
    }
    sW2[m][q][l] = make_float4(v[0], v[1], v[2], v[3]);
  }
  for (int t = tid; t < 8 * kHidden; t += kThreadsA) {
    const int o = t / kHidden, c = t % kHidden;
    sWh[o][c] = o < n_out ? p.w.W3[o * kHidden + c] : 0.0f;
    if constexpr (kCritic) sOh[o][c] = o < n_a ? p.w.W2[c * k2 + kHidden + o] : 0.0f;
  }
  if (tid < kHidden) {
    sB1[tid] = p.w.b1[tid];
    sB2[tid] = p.w.b2[tid];
  }
  if (tid < 8) sBh[tid] = tid < n_out ? p.w.b3[tid] : 0.0f;
  __syncthreads();
  int nb = 0;
  if (kTrain) nb = *p.count;
  const float inv_b = nb > 0 ? 1.0f / (float)nb : 0.0f;
  const bool ref_form = p.adv_sums != nullptr;
  const double sp_d = (kTrain && !kCritic && ref_form) ? (double)p.adv_sums[0] : 0.0;
  const double sn_d = (kTrain && !kCritic && ref_form) ? (double)p.adv_sums[1] : 0.0;
  const RefWeights ref_w = ref_weights(sp_d, sn_d, nb);
  const float lo = 1.0f - p.clip_param, hi = 1.0f + p.clip_param;
  const long long n = p.n, ntiles = (n + 31) / 32;
  constexpr int kWaves = kThreadsA / 64;
  for (long long tile = (long long)blockIdx.x * kWaves + wave; tile < ntiles; tile += (long long)gridDim.x * kWaves) {
    asm volatile("" ::: "memory");  // keep the tile-invariant LDS reads inside the persistent loop (mm_policy_mfma.h)
    const long long ag = tile * 32 + j;
    bool live = ag < n;
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
      float4 *dst = reinterpret_cast<float4 *>(p.s_xs + ag * kXs + 16 * h);
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
      if (kTrain) store_tile(p.s_h1 + ag * kHidden + 32 * m + 4 * h, h1[m]);
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
      if (kTrain) store_tile(p.s_h2 + ag * kHidden + 32 * m + 4 * h, h2[m]);
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
      if (h == 0 && ag < n && p.out0) p.out0[ag] = live ? v : 0.0f;
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
        if (h == 0 && ag < n && p.out0) p.out0[ag] = live ? lp_a : 0.0f;
        continue;
      }
      const float olp = live ? p.old_logp[ag] : 0.0f;
      const float r = expf(lp_a - olp);
      const float c = fminf(fmaxf(r, lo), hi);
      float wsel;
      if (ref_form) ppo_clip_ref(sp_d, sn_d, ref_w, lo, hi, r, c, t_loss, wsel);
      else ppo_clip_flat(live ? p.advantages[ag] : 0.0f, lo, hi, r, c, t_loss, wsel);
      const float g_lp = live ? -inv_b * wsel * r : 0.0f;  // d loss / d logp_taken
#pragma unroll
      for (int o = 0; o < 8; o++) dhead[o] = (o < n_a) ? dlogit(g_lp, logit[o], lse, o == act) : 0.0f;
      if (h == 0 && ag < n) {
        if (p.out0) p.out0[ag] = live ? lp_a : 0.0f;
        if (p.out1) p.out1[ag] = live ? r : 0.0f;
      }
    }
    {
      float4 *dst = reinterpret_cast<float4 *>(p.s_dh + ag * kDh + 8 * h);
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
      if (lane == 0) p.lossp[tile] = pl;
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
      store_tile(p.s_dz2 + ag * kHidden + 32 * m + 4 * h, h2[m]);
    }
    // ---- dz1 = (W2[:, :128]^T dz2) . [h1 > 0]: 4 output tiles x 64 k-steps, A fragments from global memory
    const unsigned vlane = opaque_lane(lane);
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {
      const f32x16 acc = dz1_tile(p.frag, mt, vlane, h2);
#pragma unroll
      for (int g = 0; g < 4; g++) {
        float4 *dst = reinterpret_cast<float4 *>(p.s_dz1 + ag * kHidden + 32 * mt + 4 * h);
        dst[2 * g] = make_float4(h1[mt][4 * g] > 0.0f ? acc[4 * g] : 0.0f, h1[mt][4 * g + 1] > 0.0f ? acc[4 * g + 1] : 0.0f,
                                 h1[mt][4 * g + 2] > 0.0f ? acc[4 * g + 2] : 0.0f, h1[mt][4 * g + 3] > 0.0f ? acc[4 * g + 3] : 0.0f);
      }
    }
  }
}

// ---- kernel B: one workgroup = one slice of samples [row0, row1), rows are whole 32-sample tiles inside n_pad
template <bool kCritic>
__global__ __launch_bounds__(kThreadsB) void policy_train_wgrad_kernel(
    const float *__restrict__ s_h1, const float *__restrict__ s_dz1, const float *__restrict__ s_h2, const float *__restrict__ s_dz2,
    const float *__restrict__ s_dh, const float *__restrict__ s_xs, long long n_pad, long long slice_rows, float *__restrict__ part) {
  wgrad_slice<4, kCritic>(s_h1, s_dz1, s_h2, s_dz2, s_dh, s_xs, n_pad, slice_rows, part);
}

// ---- kernel C: gradient element t = sum over the partial blocks in workgroup order; the last workgroup folds the loss
MM_DEV float fold(const float *__restrict__ part, int slices, int off) { return mfma::fold<Part::kSize>(part, slices, off); }

static int fold_elems(int n_s, int k2, int n_out) { return kHidden * n_s + kHidden + kHidden * k2 + kHidden + n_out * kHidden + n_out; }

// loss_mode 0: sum / B (critic); 1: -sum / B (actor, per-sample form); 2: -sum / B^2 (actor, reference form)
__global__ __launch_bounds__(256) void policy_train_fold_kernel(const float *__restrict__ part, int slices, int n_s, int k2, int n_out,
                                                                MMMlpParams gr, const double *__restrict__ lossp, long long ntiles,
                                                                const int *__restrict__ count, int loss_mode, float *__restrict__ loss) {
  if (blockIdx.x == gridDim.x - 1) {
    __shared__ double ssum[1][256];
    loss_tree<1>(lossp, ntiles, ssum);
    if (threadIdx.x == 0) {
      const double inv = inv_count(count);
      *loss = (float)(loss_mode == 0 ? ssum[0][0] * inv : (loss_mode == 1 ? -ssum[0][0] * inv : -ssum[0][0] * inv * inv));
    }
    return;
  }
  int t = blockIdx.x * 256 + threadIdx.x;
  if (t < kHidden * n_s) { const int o = t / n_s, k = t % n_s; gr.W1[t] = fold(part, slices, Part::kW1 + o * 32 + k); return; }
  t -= kHidden * n_s;
  if (t < kHidden) { gr.b1[t] = fold(part, slices, Part::kb1 + t); return; }
  t -= kHidden;
  if (t < kHidden * k2) { const int o = t / k2, k = t % k2; gr.W2[t] = fold(part, slices, Part::kW2 + o * kCat + k); return; }
  t -= kHidden * k2;
  if (t < kHidden) { gr.b2[t] = fold(part, slices, Part::kb2 + t); return; }
  t -= kHidden;
  if (t < n_out * kHidden) { gr.W3[t] = fold(part, slices, Part::kHd + t); return; }
  t -= n_out * kHidden;
  if (t < n_out) gr.b3[t] = fold(part, slices, Part::kbh + t);
}

static unsigned grid_a(long long ntiles) { return persistent_grid(ntiles, kThreadsA / 64); }

// The code object holds the kernel templates' instances in the order of their first use, and the recorded one
// (profiles/policy_train) has them in this order; the launch helpers below name them in another.
[[maybe_unused]] static const void *const kKernelOrder[] = {
    (const void *)policy_train_sample_kernel<false, false>, (const void *)policy_train_sample_kernel<true, false>,
    (const void *)policy_train_sample_kernel<false, true>,  (const void *)policy_train_wgrad_kernel<false>,
    (const void *)policy_train_sample_kernel<true, true>,   (const void *)policy_train_wgrad_kernel<true>};

// ---- host-side launch helpers (declared in mm_policy_chunked.h): the one spelling of each training launch, on the samples and
// rows the caller points at -- the whole batch for mm_policy_train below, one pass for the pass loops of mm_policy_chunked.hip
Layout layout_of(long long n) { return layout(n); }

long long critic_frag_offset() { return kFrag; }

void launch_prep(hipStream_t s, const float *W2a, const float *W2c, int k2c, float4 *frag, const uint8_t *valid, long long n,
                 int *count) {
  hipLaunchKernelGGL(policy_train_prep_kernel, dim3(2 * 4096 / 256), dim3(256), 0, s, W2a, W2c, k2c, frag, valid, n, count);
}

void launch_sample(hipStream_t s, bool critic, const PassArgs &p) {
  SampleArgs a = {};
  a.obs = p.obs; a.obs_stride = p.obs_stride; a.n = p.n; a.n_s = p.n_s; a.actions = p.actions; a.act_stride = p.act_stride;
  a.returns = p.returns; a.ret_stride = p.ret_stride; a.old_logp = p.old_logp; a.valid = p.valid; a.w = p.w; a.n_a = p.n_a;
  a.clip_param = p.clip_param; a.huber = p.huber; a.adv_sums = p.adv_sums; a.advantages = p.advantages; a.count = p.count;
  a.frag = p.frag;
  a.s_h1 = p.rows.h1; a.s_dz1 = p.rows.dz1; a.s_h2 = p.rows.h2; a.s_dz2 = p.rows.dz2; a.s_dh = p.rows.dh; a.s_xs = p.rows.xs;
  a.lossp = p.lossp; a.out0 = p.out0; a.out1 = p.out1;
  const unsigned grid = grid_a((p.n + 31) / 32);
  if (critic) hipLaunchKernelGGL((policy_train_sample_kernel<true, true>), dim3(grid), dim3(kThreadsA), 0, s, a);
  else hipLaunchKernelGGL((policy_train_sample_kernel<false, true>), dim3(grid), dim3(kThreadsA), 0, s, a);
}

void launch_wgrad(hipStream_t s, bool critic, const SampleRows &r, long long n_pad, long long slice_rows, int slices, float *part) {
  if (critic)
    hipLaunchKernelGGL((policy_train_wgrad_kernel<true>), dim3(slices), dim3(kThreadsB), 0, s, r.h1, r.dz1, r.h2, r.dz2, r.dh, r.xs,
                       n_pad, slice_rows, part);
  else
    hipLaunchKernelGGL((policy_train_wgrad_kernel<false>), dim3(slices), dim3(kThreadsB), 0, s, r.h1, r.dz1, r.h2, r.dz2, r.dh, r.xs,
                       n_pad, slice_rows, part);
}

}  // namespace pt
}  // namespace mm

extern "C" int32_t mm_policy_eval(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                  int64_t act_stride, const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic,
                                  int32_t hidden, int32_t n_a, float *logp_taken, float *value, MMStream stream) {
  using namespace mm::pt;
  if (!actor && !critic) return MM_ERR_INVALID_ARG;
  if ((actor && !complete(actor)) || (critic && !complete(critic))) return MM_ERR_INVALID_ARG;
  if (!shape_ok(n, n_s, hidden, n_a, kHidden)) return MM_ERR_INVALID_ARG;
  if (n == 0) return MM_OK;  // (empty outputs may be NULL)
  if ((actor != nullptr) != (logp_taken != nullptr) || (critic != nullptr) != (value != nullptr)) return MM_ERR_INVALID_ARG;
  if (!obs || !actions || obs_stride < n_s) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  SampleArgs a = {};
  a.obs = obs; a.obs_stride = obs_stride; a.n = n; a.n_s = n_s; a.actions = actions; a.act_stride = act_stride;
  a.valid = valid; a.n_a = n_a;
  const unsigned grid = grid_a((n + 31) / 32);
  if (actor) {
    a.w = *actor; a.out0 = logp_taken;
    hipLaunchKernelGGL((policy_train_sample_kernel<false, false>), dim3(grid), dim3(kThreadsA), 0, s, a);
  }
  if (critic) {
    a.w = *critic; a.out0 = value;
    hipLaunchKernelGGL((policy_train_sample_kernel<true, false>), dim3(grid), dim3(kThreadsA), 0, s, a);
  }
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

extern "C" int32_t mm_policy_train_scratch_bytes(int64_t n, uint64_t *bytes) {
  if (n < 0 || !bytes) return MM_ERR_INVALID_ARG;
  *bytes = (uint64_t)mm::pt::layout(n).total * 4u;
  return MM_OK;
}

extern "C" int32_t mm_policy_train(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                   int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                   const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden,
                                   int32_t n_a, float clip_param, int32_t critic_loss, const float *adv_sums, const float *advantages,
                                   const MMMlpParams *actor_grads, const MMMlpParams *critic_grads, float *loss, float *logp_taken,
                                   float *value, float *ratio, void *scratch, uint64_t scratch_bytes, MMStream stream) {
  using namespace mm::pt;
  if ((!actor && !critic) || !loss) return MM_ERR_INVALID_ARG;
  if ((actor != nullptr) != (actor_grads != nullptr) || (critic != nullptr) != (critic_grads != nullptr)) return MM_ERR_INVALID_ARG;
  if ((actor && (!complete(actor) || !complete(actor_grads))) || (critic && (!complete(critic) || !complete(critic_grads))))
    return MM_ERR_INVALID_ARG;
  if (!shape_ok(n, n_s, hidden, n_a, kHidden)) return MM_ERR_INVALID_ARG;
  if (critic_loss != MM_PT_CRITIC_MSE && critic_loss != MM_PT_CRITIC_HUBER) return MM_ERR_INVALID_ARG;
  if (!(clip_param >= 0.0f)) return MM_ERR_INVALID_ARG;
  if ((!actor && (logp_taken || ratio)) || (!critic && value)) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int k2c = kHidden + n_a;
  if (n > 0) {  // (n == 0: the per-sample inputs, adv_sums, advantages and the scratch are not looked at and may be NULL)
    if (!obs || !actions || obs_stride < n_s || (actor && !old_logp) || (critic && !returns)) return MM_ERR_INVALID_ARG;
    if (actor && ((adv_sums != nullptr) == (advantages != nullptr))) return MM_ERR_INVALID_ARG;
    if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < (uint64_t)layout(n).total * 4u) return MM_ERR_INVALID_ARG;
  }
  if (hipMemsetAsync(loss, 0, 2 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
  if (n == 0) {
    if (actor && !zero_mlp_grads(s, actor_grads, kHidden, n_s, kHidden, n_a)) return MM_ERR_DEVICE;
    if (critic && !zero_mlp_grads(s, critic_grads, kHidden, n_s, k2c, 1)) return MM_ERR_DEVICE;
    return MM_OK;
  }
  const Layout L = layout(n);
  float *sc = (float *)scratch;
  int *count = (int *)sc;
  if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess) return MM_ERR_DEVICE;
  launch_prep(s, actor ? actor->W2 : nullptr, critic ? critic->W2 : nullptr, k2c, (float4 *)(sc + L.frag), valid, n, count);
  PassArgs p = {};  // the whole batch in one pass
  p.obs = obs; p.obs_stride = obs_stride; p.n = n; p.n_s = n_s; p.actions = actions; p.act_stride = act_stride; p.returns = returns;
  p.ret_stride = ret_stride; p.old_logp = old_logp; p.valid = valid; p.n_a = n_a; p.clip_param = clip_param;
  p.huber = critic_loss == MM_PT_CRITIC_HUBER; p.adv_sums = adv_sums; p.advantages = advantages; p.count = count;
  p.rows = mm::chunked::rows_of(sc, L); p.lossp = (double *)(sc + L.lossp);
  for (int net = 0; net < 2; net++) {  // the actor's three kernels, then the critic's over the same scratch
    const MMMlpParams *w = net ? critic : actor;
    if (!w) continue;
    const int k2 = net ? k2c : kHidden, n_out = net ? 1 : n_a;
    p.w = *w; p.frag = (const float4 *)(sc + L.frag + net * kFrag);
    p.out0 = net ? value : logp_taken; p.out1 = net ? nullptr : ratio;
    launch_sample(s, net != 0, p);
    launch_wgrad(s, net != 0, p.rows, L.n_pad, L.slice_rows, L.slices, sc + L.part);
    hipLaunchKernelGGL(policy_train_fold_kernel, dim3((fold_elems(n_s, k2, n_out) + 255) / 256 + 1), dim3(256), 0, s, sc + L.part,
                       L.slices, (int)n_s, k2, n_out, net ? *critic_grads : *actor_grads, (const double *)p.lossp, L.ntiles,
                       (const int *)count, net ? 0 : (adv_sums ? 2 : 1), loss + net);
  }
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
