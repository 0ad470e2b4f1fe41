// mm_policy_wide_train.hip -- loss and parameter gradient of MAPPO's separate actor and critic at hidden size 512
// (include/mm_policy_wide_train.h), and the forward-only mm_policy_wide_eval.
//
// mm_policy_train.hip's four launches per call (prep, A, B, C) in the layout of mm_policy_mfma.h, re-cut for a layer that fits
// neither the LDS (fc2 is 1 MiB) nor the register file (a 512-wide layer of a 32-sample tile is 16 accumulator tiles):
//
//   prep      W2[:, :512]^T of each given network as a plain [512][512] array (the A operand of dz1), a copy of W2[:, :512] at
//             row pitch 512 (the A operand of fc2 where W2's own rows are not 16-byte aligned: the critic's are 512 + n_a floats
//             long), and B = the number of valid samples.
//   kernel A  one wave per 32 samples, the whole per-sample pass in one launch.  A layer is computed in four QUARTERS of four
//             accumulator tiles (128 output features, 64 registers), and its 512-long reduction is walked in 16 chunks of 32
//             features.  W2 in torch layout is A-fragment order in 16-byte pieces -- lane (i, h) needs W[32 m + i][32 c + 8 g +
//             4 h .. + 3] for k-steps 4 g .. 4 g + 3 of chunk c -- so the A operand is global_load_dwordx4 along the rows, L2
//             resident and shared through the L1 by the eight waves of a workgroup, which walk the same weights.
//               forward   chunk c of h1 is produced where it is consumed, ReLU of 16 MFMAs against W1's fragments in LDS (64 KB),
//                         16 registers that are the B operands of the chunk's 4 x 16 fc2 MFMAs: h1 is computed once per quarter
//                         (4 x 256 MFMAs on top of fc2's 4096).  Each finished quarter is stored (h2) and folded into the <= 8
//                         head sums on the VALU.  The critic's one-hot block is a column gather where the accumulator is
//                         initialised, out of an [8][512] LDS table.
//               head      log-softmax / value, the loss terms, dlogit / dvalue: mm_policy_train.hip's, from the shared helpers.
//               dz2       (W3^T dhead) . [h2 > 0] on the VALU, h2 read back from the lane's own stores.
//               dz1       the same quarter / chunk walk with W2^T as the A operand and the lane's own dz2 row as the B operand
//                         (register s of a [sample][feature] float4 walk is the B operand of k-step s), masked by the lane's
//                         own h1 row.
//             mm_policy_wide_eval is the forward and the head of the same template (!kTrain): it stores no rows, so it needs no
//             scratch, and a row's outputs are the same bits as the training call's diagnostics.
//   kernel B  contractions over the sample dimension, the sample index as the MFMA k dimension, both operands coalesced row
//             reads of the scratch.  The output is tiled over workgroups as well as the samples: blockIdx.x is the slice of
//             samples (at most 48: with the 10 output blocks that is 480 workgroups, one resident round of two per CU, and a slice's blocks
//             share an XCD's L2), blockIdx.y one of 10 output blocks = (half of the 512 rows) x (four groups of 4 column tiles of dz2^T h1 |
//             the "extra" group: the one-hot column tile of dW2, dW1 = dz1^T x, the head rows dhead^T h2 and the bias sums).
//             A wave owns 2 row tiles x 4 column tiles (8 accumulator tiles).
//   kernel C  every parameter's gradient = the partial blocks summed in slice order (fp64 running sum), written in torch
//             layout; the loss partials folded by one workgroup in a fixed tree.
// The actor's three kernels run first, then the critic's over the same scratch (stream order).
#include "mm_policy_wide_chunked.h"  // kWide, kCat, kSquare, Part, WideLayout; mm_policy_mfma.h and the public header

namespace mm {
namespace wt {

using namespace mfma;  // frag_row, mfma4, store_tile, relu, the objective's terms, count_valid, fold, loss_tree, persistent_grid

constexpr int kChunks = kWide / 32;                       // 32-feature chunks of a reduction
constexpr int kWavesA = MM_POLICY_WIDE_TRAIN_WAVES;       // 2 per SIMD
constexpr int kThreadsA = 64 * kWavesA;
constexpr int kThreadsB = 256;                            // 4 waves
constexpr int kOhPitch = kWide + 8;                       // row pitch of the one-hot column table in LDS
constexpr int kOutBlocks = 10;                            // kernel B: 2 row halves x (4 column groups + the extra group)
static_assert(MM_POLICY_WIDE_TRAIN_TILE == 32, "one MFMA tile of samples per wave");
static_assert(MM_POLICY_WIDE_TRAIN_MAX_GRID == 256, "persistent_grid launches at most one workgroup per CU");

typedef float f32x4 __attribute__((ext_vector_type(4)));

static_assert(Part::kSize * 4 == MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES, "the header states the partial block");
static_assert((32 + 4 * kWide + kDh) * 4 == MM_POLICY_WIDE_TRAIN_ROW_BYTES && kXs == 32, "the header states the rows");
static_assert(kHdr * 4 + 4 * kSquare * 4 == MM_POLICY_WIDE_TRAIN_FIXED_BYTES, "the header states the fixed part");

// The scratch of a call on n samples (WideLayout, mm_policy_wide_chunked.h)
static WideLayout layout(long long n) {
  WideLayout L;
  L.ntiles = (n + 31) / 32;
  L.n_pad = L.ntiles * 32;
  L.w2t = kHdr;
  L.w2p = L.w2t + 2 * kSquare;
  L.xs = L.w2p + 2 * kSquare;
  L.h1 = L.xs + L.n_pad * kXs;
  L.h2 = L.h1 + L.n_pad * kWide;
  L.dz2 = L.h2 + L.n_pad * kWide;
  L.dz1 = L.dz2 + L.n_pad * kWide;
  L.dh = L.dz1 + L.n_pad * kWide;
  L.lossp = L.dh + L.n_pad * kDh;  // double[ntiles]
  L.part = L.lossp + 2 * L.ntiles;
  long long tiles_per = (L.ntiles + MM_POLICY_WIDE_TRAIN_MAX_SLICES - 1) / MM_POLICY_WIDE_TRAIN_MAX_SLICES;
  if (tiles_per < MM_POLICY_WIDE_TRAIN_MIN_SLICE_TILES) tiles_per = MM_POLICY_WIDE_TRAIN_MIN_SLICE_TILES;
  L.slices = (int)((L.ntiles + tiles_per - 1) / tiles_per);
  if (L.slices < 1) L.slices = 1;
  L.slice_rows = tiles_per * 32;
  L.total = L.part + (long long)L.slices * Part::kSize;
  return L;
}

// ---- prep: element t of [network 2][512][512]: the transposed and the re-pitched copy of W2[:, :512]; the count of valid samples
constexpr int kPrepGrid = (int)(2 * kSquare / 256);
__global__ __launch_bounds__(256) void policy_wide_prep_kernel(const float *__restrict__ W2a, const float *__restrict__ W2c, int k2c,
                                                               float *__restrict__ w2t, float *__restrict__ w2p,
                                                               const uint8_t *__restrict__ valid, long long n, int *__restrict__ count) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const bool crit = t >= (int)kSquare;
  const float *W2 = crit ? W2c : W2a;
  const int k2 = crit ? k2c : kWide;
  if (W2) {
    const int e = t & ((int)kSquare - 1), r = e >> 9, c = e & (kWide - 1);
    w2p[t] = W2[r * k2 + c];  // [out r][in c]
    w2t[t] = W2[c * k2 + r];  // [in r][out c]
  }
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
  const float *W2f;  // fc2's A operand: w.W2 itself or its copy at pitch 512
  int pitch2;        // its row pitch
  int n_a;
  float clip_param;
  int huber;
  const float *adv_sums, *advantages;
  const int *count;
  const float *w2t;
  float *s_xs, *s_h1, *s_h2, *s_dz2, *s_dz1, *s_dh;
  double *lossp;
  float *out0, *out1;  // actor: logp_taken, ratio; critic: value, unused
};

// four consecutive k-steps' A fragments: one 16-byte load, or four 4-byte loads where the rows are not 16-byte aligned
template <bool kVec>
MM_DEV float4 load_frag(const float *p) {
  if constexpr (kVec) {
    const f32x4 v = *reinterpret_cast<const f32x4 *>(p);
    return make_float4(v.x, v.y, v.z, v.w);
  } else {
    return make_float4(p[0], p[1], p[2], p[3]);
  }
}

// one 32-feature chunk of the reduction into a quarter's four accumulator tiles.  a = W + (128 q + i) * pitch + 32 c + 4 h: the
// lane's piece of output row i of tile 0; b: the chunk's B operands, register s = input feature 32 c + frag_row(s, h)
template <bool kVec>
MM_DEV void chunk_mma(f32x16 (&acc)[4], const float *a, long long pitch, const f32x16 &b) {
#pragma unroll
  for (int g = 0; g < 4; g++)
#pragma unroll
    for (int m = 0; m < 4; m++)
      acc[m] = mfma4(load_frag<kVec>(a + 32 * m * pitch + 8 * g), b[4 * g + 0], b[4 * g + 1], b[4 * g + 2], b[4 * g + 3], acc[m]);
}

// the lane's 16 floats of a 32-feature piece of a [sample][feature] row, in accumulator-register order; src = row + 32 m + 4 h
MM_DEV f32x16 load_tile(const float *src) {
  f32x16 t;
  const f32x4 *s = reinterpret_cast<const f32x4 *>(src);
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const f32x4 v = s[2 * g];
    t[4 * g] = v.x; t[4 * g + 1] = v.y; t[4 * g + 2] = v.z; t[4 * g + 3] = v.w;
  }
  return t;
}

// ---- kernel A
template <bool kCritic, bool kTrain, bool kVec>
__global__ __launch_bounds__(kThreadsA) void policy_wide_sample_kernel(const SampleArgs p) {
  __shared__ float4 sW1[kChunks][4][64];  // [chunk = out tile][k-step / 4][lane]: 64 KB
  __shared__ __attribute__((aligned(16))) float sWh[8][kWide];  // head rows (zero past the head's width): 16 KB
  __shared__ __attribute__((aligned(16))) float sOh[kCritic ? 8 : 1][kOhPitch];  // critic: fc2's one-hot columns, [action][feature]
  __shared__ __attribute__((aligned(16))) float sB1[kWide], sB2[kWide];
  __shared__ float sBh[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int n_s = p.n_s, n_a = p.n_a;
  const int k2 = kCritic ? kWide + n_a : kWide;  // fc2's row length in w.W2
  const int n_out = kCritic ? 1 : n_a;
  for (int t = tid; t < kChunks * 4 * 64; t += kThreadsA) {
    const int l = t & 63, q = (t >> 6) & 3, m = t >> 8;
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = 2 * (4 * q + u) + (l >> 5);
      v[u] = k < n_s ? p.w.W1[(32 * m + (l & 31)) * n_s + k] : 0.0f;
    }
    sW1[m][q][l] = make_float4(v[0], v[1], v[2], v[3]);
  }
  for (int t = tid; t < 8 * kWide; t += kThreadsA) {
    const int o = t / kWide, c = t % kWide;
    sWh[o][c] = o < n_out ? p.w.W3[o * kWide + c] : 0.0f;
    if constexpr (kCritic) sOh[o][c] = o < n_a ? p.w.W2[c * k2 + kWide + o] : 0.0f;
  }
  for (int t = tid; t < kWide; t += kThreadsA) {
    sB1[t] = p.w.b1[t];
    sB2[t] = p.w.b2[t];
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
  const long long pitch2 = p.pitch2;
  for (long long tile = (long long)blockIdx.x * kWavesA + wave; tile < ntiles; tile += (long long)gridDim.x * kWavesA) {
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
    // ---- forward: fc2 quarter by quarter, h1's chunk made where it is used; the head sums (before the cross-half add)
    float hs[8];
#pragma unroll
    for (int o = 0; o < 8; o++) hs[o] = 0.0f;
#pragma unroll 1
    for (int q = 0; q < 4; q++) {
      f32x16 acc[4];
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int f = 128 * q + 32 * m + 8 * g + 4 * h;
          float4 b = *reinterpret_cast<const float4 *>(&sB2[f]);
          if constexpr (kCritic) {  // the one-hot block of fc2: column 512 + act
            const float4 o = *reinterpret_cast<const float4 *>(&sOh[act][f]);
            b.x += o.x; b.y += o.y; b.z += o.z; b.w += o.w;
          }
          acc[m][4 * g] = b.x; acc[m][4 * g + 1] = b.y; acc[m][4 * g + 2] = b.z; acc[m][4 * g + 3] = b.w;
        }
      const float *arow = p.W2f + (128 * q + j) * pitch2 + 4 * h;
#pragma unroll 1
      for (int c = 0; c < kChunks; c++) {
        f32x16 a1;
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const float4 b = *reinterpret_cast<const float4 *>(&sB1[32 * c + 8 * g + 4 * h]);
          a1[4 * g] = b.x; a1[4 * g + 1] = b.y; a1[4 * g + 2] = b.z; a1[4 * g + 3] = b.w;
        }
#pragma unroll
        for (int s = 0; s < 4; s++) a1 = mfma4(sW1[c][s][lane], x[4 * s + 0], x[4 * s + 1], x[4 * s + 2], x[4 * s + 3], a1);
        const f32x16 h1c = relu(a1);
        if (kTrain && q == 0) store_tile(p.s_h1 + ag * kWide + 32 * c + 4 * h, h1c);
        chunk_mma<kVec>(acc, arow + 32 * c, pitch2, h1c);
      }
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const f32x16 h2 = relu(acc[m]);
        if (kTrain) store_tile(p.s_h2 + ag * kWide + 128 * q + 32 * m + 4 * h, h2);
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int f = 128 * q + 32 * m + 8 * g + 4 * h;
#pragma unroll
          for (int o = 0; o < (kCritic ? 1 : 8); o++) {  // rows past the head's width are zero in sWh
            const float4 wa = *reinterpret_cast<const float4 *>(&sWh[o][f]);
            hs[o] = fmaf(h2[4 * g + 0], wa.x, hs[o]);
            hs[o] = fmaf(h2[4 * g + 1], wa.y, hs[o]);
            hs[o] = fmaf(h2[4 * g + 2], wa.z, hs[o]);
            hs[o] = fmaf(h2[4 * g + 3], wa.w, hs[o]);
          }
        }
      }
    }
    // ---- head, the objective's per-sample terms, dhead (both lane halves compute the same numbers)
    float dhead[8];
    double t_loss = 0.0;
    if (kCritic) {
      const float v = hs[0] + __shfl_xor(hs[0], 32, 64) + sBh[0];
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
        const float s = hs[o] + __shfl_xor(hs[o], 32, 64);
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
    if constexpr (kTrain) {
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
      // ---- dz2 = (W3^T dhead) . [h2 > 0]: the lane's own pieces of its h2 row, four floats at a time
#pragma unroll 4
      for (int t = 0; t < 4 * kChunks; t++) {
        const int f = 8 * t + 4 * h;
        const f32x4 h2v = *reinterpret_cast<const f32x4 *>(p.s_h2 + ag * kWide + f);
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
        for (int o = 0; o < (kCritic ? 1 : 8); o++) {  // rows past the head's width are zero in sWh and their dhead is zero
          const float4 wa = *reinterpret_cast<const float4 *>(&sWh[o][f]);
          s0 = fmaf(dhead[o], wa.x, s0);
          s1 = fmaf(dhead[o], wa.y, s1);
          s2 = fmaf(dhead[o], wa.z, s2);
          s3 = fmaf(dhead[o], wa.w, s3);
        }
        *reinterpret_cast<float4 *>(p.s_dz2 + ag * kWide + f) =
            make_float4(h2v.x > 0.0f ? s0 : 0.0f, h2v.y > 0.0f ? s1 : 0.0f, h2v.z > 0.0f ? s2 : 0.0f, h2v.w > 0.0f ? s3 : 0.0f);
      }
      // ---- dz1 = (W2[:, :512]^T dz2) . [h1 > 0]: the forward's walk, A = W2^T rows, B = the lane's own dz2 row
#pragma unroll 1
      for (int q = 0; q < 4; q++) {
        f32x16 acc[4];
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
          for (int r = 0; r < 16; r++) acc[m][r] = 0.0f;
        const float *arow = p.w2t + (128 * q + j) * (long long)kWide + 4 * h;
#pragma unroll 1
        for (int c = 0; c < kChunks; c++) {
          const f32x16 b = load_tile(p.s_dz2 + ag * kWide + 32 * c + 4 * h);
          chunk_mma<true>(acc, arow + 32 * c, kWide, b);
        }
#pragma unroll
        for (int m = 0; m < 4; m++) {
          const f32x16 h1t = load_tile(p.s_h1 + ag * kWide + 128 * q + 32 * m + 4 * h);
          f32x16 d;
#pragma unroll
          for (int r = 0; r < 16; r++) d[r] = h1t[r] > 0.0f ? acc[m][r] : 0.0f;
          store_tile(p.s_dz1 + ag * kWide + 128 * q + 32 * m + 4 * h, d);
        }
      }
    }
  }
}

// ---- kernel B: workgroup (slice = blockIdx.x, output block = blockIdx.y); rows [row0, row1) are whole 32-sample tiles inside n_pad
template <bool kCritic>
__global__ __launch_bounds__(kThreadsB) void policy_wide_wgrad_kernel(
    const float *__restrict__ s_xs, const float *__restrict__ s_h1, const float *__restrict__ s_h2, const float *__restrict__ s_dz2,
    const float *__restrict__ s_dz1, const float *__restrict__ s_dh, long long n_pad, long long slice_rows, float *__restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, kh = lane >> 5;
  const int rb = blockIdx.y / 5, cg = blockIdx.y % 5;
  const int rt0 = 8 * rb + 2 * wave;  // the wave's two row tiles: output rows 32 rt0 .. 32 rt0 + 63
  const long long row0 = (long long)blockIdx.x * slice_rows;
  long long row1 = row0 + slice_rows;
  if (row1 > n_pad) row1 = n_pad;
  float *out = part + (long long)blockIdx.x * Part::kSize;
  if (cg < 4) {  // dW2[:, 128 cg .. 128 cg + 127] = dz2^T h1
    f32x16 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int c = 0; c < 4; c++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[t][c][r] = 0.0f;
    for (long long rbase = row0 + kh; rbase < row1; rbase += 2 * kUnrollB)  // (a slice is a whole number of 32-sample tiles)
#pragma unroll
      for (int u = 0; u < kUnrollB; u++) {
        const long long row = rbase + 2 * u;
        float a[2], b[4];
#pragma unroll
        for (int t = 0; t < 2; t++) a[t] = s_dz2[row * kWide + 32 * (rt0 + t) + i];
#pragma unroll
        for (int c = 0; c < 4; c++) b[c] = s_h1[row * kWide + 128 * cg + 32 * c + i];
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
          for (int c = 0; c < 4; c++) acc[t][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[c], acc[t][c], 0, 0, 0);
      }
    // accumulator register r of lane (j = i, h = kh): output row frag_row(r, kh), column j
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int c = 0; c < 4; c++)
#pragma unroll
        for (int r = 0; r < 16; r++)
          out[Part::kW2 + (32 * (rt0 + t) + frag_row(r, kh)) * kCat + 128 * cg + 32 * c + i] = acc[t][c][r];
  } else {  // the extra group: dW2's one-hot tile, dW1 = dz1^T x, the head rows dhead^T h2[:, the wave's columns], the bias sums
    f32x16 aoh[2], aw1[2], ahd[2];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int r = 0; r < 16; r++) { aoh[t][r] = 0.0f; aw1[t][r] = 0.0f; ahd[t][r] = 0.0f; }
    double bs2[2] = {}, bs1[2] = {}, bsh = 0.0;
    for (long long rbase = row0 + kh; rbase < row1; rbase += 2 * kUnrollB)
#pragma unroll
      for (int u = 0; u < kUnrollB; u++) {
        const long long row = rbase + 2 * u;
        const float ah = i < kDh ? s_dh[row * kDh + i] : 0.0f;
        const float bx = s_xs[row * kXs + i];
        float boh = 0.0f;
        if (kCritic) boh = (float)i == s_dh[row * kDh + kActCol] ? 1.0f : 0.0f;  // one_hot(action) row
        float a2[2], a1[2], bh[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
          a2[t] = s_dz2[row * kWide + 32 * (rt0 + t) + i];
          a1[t] = s_dz1[row * kWide + 32 * (rt0 + t) + i];
          bh[t] = s_h2[row * kWide + 32 * (rt0 + t) + i];
        }
#pragma unroll
        for (int t = 0; t < 2; t++) {
          if (kCritic) aoh[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[t], boh, aoh[t], 0, 0, 0);
          aw1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[t], bx, aw1[t], 0, 0, 0);
          ahd[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ah, bh[t], ahd[t], 0, 0, 0);
          bs2[t] += (double)a2[t];
          bs1[t] += (double)a1[t];
        }
        bsh += (double)ah;
      }
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const int rt = rt0 + t;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        if (kCritic) out[Part::kW2 + (32 * rt + frag_row(r, kh)) * kCat + kWide + i] = aoh[t][r];
        out[Part::kW1 + (32 * rt + frag_row(r, kh)) * 32 + i] = aw1[t][r];
      }
#pragma unroll
      for (int r = 0; r < 8; r++) out[Part::kHd + frag_row(r, kh) * kWide + 32 * rt + i] = ahd[t][r];  // rows 0..15
      const double s2 = bs2[t] + __shfl_xor(bs2[t], 32, 64);
      const double s1 = bs1[t] + __shfl_xor(bs1[t], 32, 64);
      if (kh == 0) {
        out[Part::kb2 + 32 * rt + i] = (float)s2;
        out[Part::kb1 + 32 * rt + i] = (float)s1;
      }
    }
    bsh += __shfl_xor(bsh, 32, 64);
    if (kh == 0 && rt0 == 0 && i < kDh) out[Part::kbh + i] = (float)bsh;
  }
}

// ---- kernel C: gradient element t = sum over the partial blocks in slice order; the last workgroup folds the loss
MM_DEV float fold_w(const float *__restrict__ part, int slices, int off) { return mfma::fold<Part::kSize>(part, slices, off); }

static int fold_elems(int n_s, int k2, int n_out) { return kWide * n_s + kWide + kWide * k2 + kWide + n_out * kWide + n_out; }

// loss_mode 0: sum / B (critic); 1: -sum / B (actor, per-sample form); 2: -sum / B^2 (actor, reference form)
__global__ __launch_bounds__(256) void policy_wide_fold_kernel(const float *__restrict__ part, int slices, int n_s, int k2, int n_out,
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
  if (t < kWide * n_s) { const int o = t / n_s, k = t % n_s; gr.W1[t] = fold_w(part, slices, Part::kW1 + o * 32 + k); return; }
  t -= kWide * n_s;
  if (t < kWide) { gr.b1[t] = fold_w(part, slices, Part::kb1 + t); return; }
  t -= kWide;
  if (t < kWide * k2) { const int o = t / k2, k = t % k2; gr.W2[t] = fold_w(part, slices, Part::kW2 + o * kCat + k); return; }
  t -= kWide * k2;
  if (t < kWide) { gr.b2[t] = fold_w(part, slices, Part::kb2 + t); return; }
  t -= kWide;
  if (t < n_out * kWide) { gr.W3[t] = fold_w(part, slices, Part::kHd + t); return; }
  t -= n_out * kWide;
  if (t < n_out) gr.b3[t] = fold_w(part, slices, Part::kbh + t);
}

static unsigned grid_a(long long ntiles) { return persistent_grid(ntiles, kWavesA); }

// fc2's rows can be read 16 bytes at a time
static bool vec_rows(const float *W2, int pitch) { return ((uintptr_t)W2 & 15) == 0 && (pitch & 3) == 0; }

template <bool kCritic, bool kTrain>
static void launch_sample(hipStream_t s, unsigned grid, const SampleArgs &a) {
  if (vec_rows(a.W2f, a.pitch2))
    hipLaunchKernelGGL((policy_wide_sample_kernel<kCritic, kTrain, true>), dim3(grid), dim3(kThreadsA), 0, s, a);
  else
    hipLaunchKernelGGL((policy_wide_sample_kernel<kCritic, kTrain, false>), dim3(grid), dim3(kThreadsA), 0, s, a);
}

// ---- host-side launch helpers (declared in mm_policy_wide_chunked.h): the one spelling of each training launch, on the samples
// and rows the caller points at -- the whole batch for mm_policy_wide_train below, one pass for mm_policy_wide_chunked.hip
WideLayout layout_of(long long n) { return layout(n); }

void launch_prep(hipStream_t s, const float *W2a, const float *W2c, int k2c, float *w2t, float *w2p, const uint8_t *valid, long long n,
                 int *count) {
  hipLaunchKernelGGL(policy_wide_prep_kernel, dim3(kPrepGrid), dim3(256), 0, s, W2a, W2c, k2c, w2t, w2p, valid, n, count);
}

void launch_sample(hipStream_t s, bool critic, const PassArgs &p) {
  SampleArgs a = {};
  a.obs = p.obs; a.obs_stride = p.obs_stride; a.n = p.n; a.n_s = p.n_s; a.actions = p.actions; a.act_stride = p.act_stride;
  a.returns = p.returns; a.ret_stride = p.ret_stride; a.old_logp = p.old_logp; a.valid = p.valid; a.w = p.w; a.n_a = p.n_a;
  a.clip_param = p.clip_param; a.huber = p.huber; a.adv_sums = p.adv_sums; a.advantages = p.advantages; a.count = p.count;
  a.w2t = p.w2t;
  const int k2 = critic ? kWide + p.n_a : kWide;
  const bool in_place = vec_rows(p.w.W2, k2);
  a.W2f = in_place ? p.w.W2 : p.w2p;
  a.pitch2 = in_place ? k2 : kWide;
  a.s_xs = p.rows.xs; a.s_h1 = p.rows.h1; a.s_h2 = p.rows.h2; a.s_dz2 = p.rows.dz2; a.s_dz1 = p.rows.dz1; a.s_dh = p.rows.dh;
  a.lossp = p.lossp; a.out0 = p.out0; a.out1 = p.out1;
  const unsigned grid = grid_a((p.n + 31) / 32);
  if (critic) launch_sample<true, true>(s, grid, a);
  else launch_sample<false, true>(s, grid, a);
}

void launch_wgrad(hipStream_t s, bool critic, const WideRows &r, long long n_pad, long long slice_rows, int slices, float *part) {
  const dim3 grid_b(slices, kOutBlocks);
  if (critic)
    hipLaunchKernelGGL((policy_wide_wgrad_kernel<true>), grid_b, dim3(kThreadsB), 0, s, r.xs, r.h1, r.h2, r.dz2, r.dz1, r.dh, n_pad,
                       slice_rows, part);
  else
    hipLaunchKernelGGL((policy_wide_wgrad_kernel<false>), grid_b, dim3(kThreadsB), 0, s, r.xs, r.h1, r.h2, r.dz2, r.dz1, r.dh, n_pad,
                       slice_rows, part);
}

}  // namespace wt
}  // namespace mm

extern "C" int32_t mm_policy_wide_eval(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                       int64_t act_stride, const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic,
                                       int32_t hidden, int32_t n_a, float *logp_taken, float *value, MMStream stream) {
  using namespace mm::wt;
  if (!actor && !critic) return MM_ERR_INVALID_ARG;
  if ((actor && !complete(actor)) || (critic && !complete(critic))) return MM_ERR_INVALID_ARG;
  if (!shape_ok(n, n_s, hidden, n_a, kWide)) return MM_ERR_INVALID_ARG;
  if (n == 0) return MM_OK;  // (empty outputs may be NULL)
  if ((actor != nullptr) != (logp_taken != nullptr) || (critic != nullptr) != (value != nullptr)) return MM_ERR_INVALID_ARG;
  if (!obs || !actions || obs_stride < n_s) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  SampleArgs a = {};
  a.obs = obs; a.obs_stride = obs_stride; a.n = n; a.n_s = n_s; a.actions = actions; a.act_stride = act_stride;
  a.valid = valid; a.n_a = n_a;
  const unsigned grid = grid_a((n + 31) / 32);
  if (actor) {
    a.w = *actor; a.W2f = actor->W2; a.pitch2 = kWide; a.out0 = logp_taken;
    launch_sample<false, false>(s, grid, a);
  }
  if (critic) {
    a.w = *critic; a.W2f = critic->W2; a.pitch2 = kWide + n_a; a.out0 = value;
    launch_sample<true, false>(s, grid, a);
  }
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

extern "C" int32_t mm_policy_wide_train_scratch_bytes(int64_t n, uint64_t *bytes) {
  if (n < 0 || !bytes) return MM_ERR_INVALID_ARG;
  *bytes = (uint64_t)mm::wt::layout(n).total * 4u;
  return MM_OK;
}

extern "C" int32_t mm_policy_wide_train(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                        int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                        const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden,
                                        int32_t n_a, float clip_param, int32_t critic_loss, const float *adv_sums,
                                        const float *advantages, const MMMlpParams *actor_grads, const MMMlpParams *critic_grads,
                                        float *loss, float *logp_taken, float *value, float *ratio, void *scratch,
                                        uint64_t scratch_bytes, MMStream stream) {
  using namespace mm::wt;
  // every argument check comes before the first enqueue: a refused call writes nothing
  if ((!actor && !critic) || !loss) return MM_ERR_INVALID_ARG;
  if ((actor != nullptr) != (actor_grads != nullptr) || (critic != nullptr) != (critic_grads != nullptr)) return MM_ERR_INVALID_ARG;
  if ((actor && (!complete(actor) || !complete(actor_grads))) || (critic && (!complete(critic) || !complete(critic_grads))))
    return MM_ERR_INVALID_ARG;
  if (!shape_ok(n, n_s, hidden, n_a, kWide)) return MM_ERR_INVALID_ARG;
  if (critic_loss != MM_PT_CRITIC_MSE && critic_loss != MM_PT_CRITIC_HUBER) return MM_ERR_INVALID_ARG;
  if (!(clip_param >= 0.0f)) return MM_ERR_INVALID_ARG;
  if ((!actor && (logp_taken || ratio)) || (!critic && value)) return MM_ERR_INVALID_ARG;
  const WideLayout L = layout(n);
  if (n > 0) {  // (n == 0: the per-sample inputs, adv_sums, advantages and the scratch are not looked at and may be NULL)
    if (!obs || !actions || obs_stride < n_s || (actor && !old_logp) || (critic && !returns)) return MM_ERR_INVALID_ARG;
    if (actor && ((adv_sums != nullptr) == (advantages != nullptr))) return MM_ERR_INVALID_ARG;
    if (!scratch || ((uintptr_t)scratch & (MM_POLICY_WIDE_TRAIN_SCRATCH_ALIGN - 1)) || scratch_bytes < (uint64_t)L.total * 4u)
      return MM_ERR_INVALID_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const int k2c = kWide + n_a;
  if (hipMemsetAsync(loss, 0, 2 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
  if (n == 0) {
    if (actor && !zero_mlp_grads(s, actor_grads, kWide, n_s, kWide, n_a)) return MM_ERR_DEVICE;
    if (critic && !zero_mlp_grads(s, critic_grads, kWide, n_s, k2c, 1)) return MM_ERR_DEVICE;
    return MM_OK;
  }
  float *sc = (float *)scratch;
  int *count = (int *)sc;
  if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess) return MM_ERR_DEVICE;
  launch_prep(s, actor ? actor->W2 : nullptr, critic ? critic->W2 : nullptr, k2c, sc + L.w2t, sc + L.w2p, valid, n, count);
  PassArgs p = {};  // the whole batch in one pass
  p.obs = obs; p.obs_stride = obs_stride; p.n = n; p.n_s = n_s; p.actions = actions; p.act_stride = act_stride; p.returns = returns;
  p.ret_stride = ret_stride; p.old_logp = old_logp; p.valid = valid; p.n_a = n_a; p.clip_param = clip_param;
  p.huber = critic_loss == MM_PT_CRITIC_HUBER; p.adv_sums = adv_sums; p.advantages = advantages; p.count = count;
  const WideRows rows = {sc + L.xs, sc + L.h1, sc + L.h2, sc + L.dz2, sc + L.dz1, sc + L.dh};
  p.rows = rows; p.lossp = (double *)(sc + L.lossp);
  for (int net = 0; net < 2; net++) {  // the actor's three kernels, then the critic's over the same scratch
    const MMMlpParams *w = net ? critic : actor;
    if (!w) continue;
    const int k2 = net ? k2c : kWide, n_out = net ? 1 : n_a;
    p.w = *w; p.w2t = sc + L.w2t + net * kSquare; p.w2p = sc + L.w2p + net * kSquare;
    p.out0 = net ? value : logp_taken; p.out1 = net ? nullptr : ratio;
    launch_sample(s, net != 0, p);
    launch_wgrad(s, net != 0, rows, L.n_pad, L.slice_rows, L.slices, sc + L.part);
    hipLaunchKernelGGL(policy_wide_fold_kernel, dim3((fold_elems(n_s, k2, n_out) + 255) / 256 + 1), dim3(256), 0, s, sc + L.part,
                       L.slices, (int)n_s, k2, n_out, net ? *critic_grads : *actor_grads, (const double *)p.lossp, L.ntiles,
                       (const int *)count, net ? 0 : (adv_sums ? 2 : 1), loss + net);
  }
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
