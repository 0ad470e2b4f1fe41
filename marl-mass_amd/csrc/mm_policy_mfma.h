// mm_policy_mfma.h -- what the policy kernel files share (mm_policy_gi.hip, mm_policy_gi_train.hip, mm_policy_train.hip, the
// hidden-512 files, the bank's), and at its end the small host helpers of the training entries (argument checks, the n == 0 path).
// The device helpers are force-inlined and parametrised by compile-time sizes alone: the kernels that use them keep their
// names, their shared memory and their register budget (255 / 256 VGPRs, no spills), and no floating-point operation moves.
//
// The layout.  Every layer is computed transposed, H_out^T [feature x sample] = W [out x in] . H_in^T, one wave per 32 samples,
// on f32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32 products and sums).  The A operand of k-step s is
// A[i = lane & 31][k = lane >> 5] = W[32 m + i][2 s + (lane >> 5)], the B operand B[k = lane >> 5][j = lane & 31] the input
// feature 2 s + (lane >> 5) of sample j.  An accumulator tile has the sample on the lane and 16 features in the registers:
// lane (j, h = lane >> 5) holds feature frag_row(r, h) = (r & 3) + 8 (r >> 2) + 4 h of the tile in register r.  Walking a
// 32-feature chunk of the reduction in THAT order -- k-step s of the chunk multiplies features frag_row(s, 0) and frag_row(s, 1)
// -- makes register s of an accumulator tile directly the B operand of k-step s of the next layer: activations never leave the
// register file, and the weights are staged once per workgroup in the matching "fragment order" (stage_w2, w2t_fragment).
// Four consecutive k-steps of one lane are one float4 of fragments: one conflict-free ds_read_b128 (or one global_load_dwordx4)
// per four MFMAs (mfma4).  Registers 4 g .. 4 g + 3 of a tile are features 8 g + 4 h .. + 3, contiguous in a [sample][feature]
// row: a tile is stored as four float4 (store_tile), and a head row is read as ds_read_b128 where it is walked that way.
//
// How the helpers are cut.  A force-inlined helper is simplified on its own before it is inlined, without what the kernel knows
// about its arguments, and the sample kernels sit at the register limit: a helper is shared only in a form that leaves their
// machine code as it was.  Hence thread-derived indices are taken from threadIdx inside a helper or as unsigned (a plain int
// argument loses its range), the per-logit terms (exp_shifted, dlogit) are per-element with the 8-way loop in the kernel, and
// three pieces stay in the kernels: the value head's dot product (head_dot's FMAs with the row fixed), fc2's staging in
// mm_policy_sample.h (its row pitch is not a constant there) and the per-tile loss butterfly.
// A whole kernel body is shared as the kernel template itself, with a policy type for what differs, not as a helper
// (mm_policy_sample.h, kernel A of mm_policy_train.hip and of the bank).  Measured by cross-compiling for gfx950: with the body in a
// force-inlined function template that the kernel calls, mm_policy_train.hip's kernel A <actor, train> goes from 255 VGPRs / 71
// spilled SGPR lanes to 253 / 64 and <critic, train> from 232 / 18 to 233 / 16; as the kernel template, with a policy of trivial
// members, all eight kernels of that file are instruction for instruction the recorded ones.  The arguments stay the kernels' own
// by-value blocks (a parameter pack): the bank's two blocks joined into one struct, at the same offsets, move its SGPR figures
// (<critic, eval> 80 -> 79, <actor, train> 117 -> 89 spilled lanes); as two arguments all its figures are the recorded ones.  What
// the bank's policy computes once in its constructor matters as well: with its workgroup index and count read from the table per
// use, VGPRs move (<critic, train> 246 -> 233, measured in the joined-struct form).
// Kernel C stays written out in both files: as a force-inlined helper its index map changes policy_train_fold_kernel's code.
//
// A persistent kernel's tile loop starts with `asm volatile("" ::: "memory")`: the weight fragments are tile-invariant, and
// without the fence the compiler hoists their LDS reads out of the loop, which costs 320 registers and spills the activations.
#ifndef MM_POLICY_MFMA_H
#define MM_POLICY_MFMA_H
#include "mm_device.h"
#include "../../include/mm_policy_gi_train.h"  // MMGiParams
#include "../../include/mm_policy_train.h"     // MMMlpParams

namespace mm {
namespace mfma {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kHidden = 128;     // width of fc2's output and of every head's input
constexpr int kMaxSlices = 512;  // workgroups of kernel B = partial blocks (2 per CU)
constexpr int kUnrollB = 4;      // k-steps of kernel B whose loads are issued together
static_assert(32 % (2 * kUnrollB) == 0, "kernel B walks a slice of whole 32-sample tiles in blocks of 2 * kUnrollB rows");
constexpr int kDh = 16, kXs = 32;  // row pitch of the head-gradient rows and of the input rows of the scratch
constexpr int kActCol = 15;        // column of the head-gradient row that carries the critic's action (one-hot tile of kernel B)
constexpr int kW2Pitch = 160;      // row pitch of the dW2 partial: 5 column tiles (GI's cat(out1, out2, out3); MAPPO's 128 + one-hot)
constexpr long long kHdr = 64;     // scratch header, in floats: [0] (int) B, the number of valid samples

MM_DEV int frag_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Kernel B's slicing of ntiles 32-sample tiles (an int or a long long): whole tiles, at least 2 per slice, at most kMaxSlices slices
template <typename T>
__host__ __device__ inline T tiles_per_slice(T ntiles) {
  const T per = (ntiles + kMaxSlices - 1) / kMaxSlices;
  return per < 2 ? 2 : per;
}

// GI layer-1 fragment q -> (output tile m, k-step s): tile 0 = fc11 (3 k-steps), tiles 1-2 = fc12, 3-4 = fc13 (5 k-steps each)
MM_DEV void l1_step(int q, int &m, int &s) {
  if (q < 3) { m = 0; s = q; }
  else { m = 1 + (q - 3) / 5; s = (q - 3) % 5; }
}

// ---- four k-steps fed by one float4 of A fragments
MM_DEV f32x16 mfma4(const float4 a, float b0, float b1, float b2, float b3, f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b2, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b3, acc, 0, 0, 0);
  return acc;
}

// accumulator tile -> the lane's 16 features of a [sample][feature] row; dst = row + 32 m + 4 h
MM_DEV void store_tile(float *dst, const f32x16 &t) {
  float4 *d = reinterpret_cast<float4 *>(dst);
#pragma unroll
  for (int g = 0; g < 4; g++) d[2 * g] = make_float4(t[4 * g], t[4 * g + 1], t[4 * g + 2], t[4 * g + 3]);
}

// ---- fc2's first 32 * kGroups / 4 columns into LDS in A-fragment order: [out tile][k-step / 4][lane]
template <int kGroups, int kThreads>
MM_DEV void stage_w2(float4 (&sW2)[4][kGroups][64], const float *W2, int pitch) {
  for (unsigned t = threadIdx.x; t < 4 * kGroups * 64; t += kThreads) {
    const int l = t & 63, q = (t >> 6) % kGroups, m = t / (kGroups * 64);
    float w[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int s = 4 * q + u;  // k-step: 32-feature chunk s >> 4, step in chunk s & 15
      w[u] = W2[(32 * m + (l & 31)) * pitch + 32 * (s >> 4) + frag_row(s & 15, l >> 5)];
    }
    sW2[m][q][l] = make_float4(w[0], w[1], w[2], w[3]);
  }
}

// ---- one fc2 output tile: the bias-initialised accumulator + kChunks x 4 mfma4 over the input tiles
template <int kChunks>
MM_DEV f32x16 fc2_tile(const float4 (&sW2m)[4 * kChunks][64], const f32x16 (&h1)[kChunks], int lane, f32x16 acc) {
#pragma unroll
  for (int c = 0; c < kChunks; c++) {
#pragma unroll
    for (int q = 0; q < 4; q++)
      acc = mfma4(sW2m[4 * c + q][lane], h1[c][4 * q + 0], h1[c][4 * q + 1], h1[c][4 * q + 2], h1[c][4 * q + 3], acc);
  }
  return acc;
}

MM_DEV f32x16 relu(const f32x16 &acc) {
  f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; r++) o[r] = fmaxf(acc[r], 0.0f);
  return o;
}

// ---- one head row (before its bias): 64 FMAs per lane over the lane's features of h2, then the cross-half add
MM_DEV float head_dot(const f32x16 (&h2)[4], const float *wrow, int h, bool on) {
  float p = 0.0f;
  if (on) {
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
      for (int r = 0; r < 16; r++) p = fmaf(h2[m][r], wrow[32 * m + frag_row(r, h)], p);
  }
  return p + __shfl_xor(p, 32, 64);
}

// ---- log-softmax over the n_a <= 8 logits (fp32): lse = mx + log(sum_o exp_shifted(logit[o], mx, o < n_a)), mx = max8(logit)
MM_DEV float max8(const float (&logit)[8]) {
  float mx = logit[0];
#pragma unroll
  for (int o = 1; o < 8; o++) mx = fmaxf(mx, logit[o]);
  return mx;
}

MM_DEV float exp_shifted(float x, float mx, bool on) { return on ? expf(x - mx) : 0.0f; }

MM_DEV float logp_taken(const float (&logit)[8], float lse, int act) {
  float lp_a = 0.0f;
#pragma unroll
  for (int o = 0; o < 8; o++) lp_a = (o == act) ? logit[o] - lse : lp_a;
  return lp_a;
}

// ---- the objective's per-sample terms
// PPO-clip.  actor loss = -(1 / B^2) sum_j [S+ min(r, c) + S- max(r, c)] (reference form) or -(1 / B) sum_j [A+ min + A- max],
// c = clip(r, lo, hi).  t: the sample's term of the sum; wsel: the weight that reaches d / dr, the positive one up to 1 + clip,
// the negative one from 1 - clip.
// Reference form: S+ and S- are large and nearly cancel while every sample inside the clip band is weighted by their SUM, so
// the three possible weights are formed once in fp64 (the sum before the rounding, not after).
struct RefWeights {
  float wp, wn, wb;  // S+ / B, S- / B, (S+ + S-) / B
};

MM_DEV RefWeights ref_weights(double sp_d, double sn_d, int nb) {
  const double inv_b_d = nb > 0 ? 1.0 / (double)nb : 0.0;
  RefWeights w;
  w.wp = (float)(sp_d * inv_b_d);
  w.wn = (float)(sn_d * inv_b_d);
  w.wb = (float)((sp_d + sn_d) * inv_b_d);
  return w;
}

MM_DEV void ppo_clip_ref(double sp_d, double sn_d, const RefWeights w, float lo, float hi, float r, float c, double &t, float &wsel) {
  t = sp_d * (double)fminf(r, c) + sn_d * (double)fmaxf(r, c);
  wsel = r > hi ? w.wn : (r < lo ? w.wp : w.wb);
}

MM_DEV void ppo_clip_flat(float adv, float lo, float hi, float r, float c, double &t, float &wsel) {
  const float wp = fmaxf(adv, 0.0f), wn = fminf(adv, 0.0f);  // one of them is zero
  t = (double)wp * (double)fminf(r, c) + (double)wn * (double)fmaxf(r, c);
  wsel = (r <= hi ? wp : 0.0f) + (r >= lo ? wn : 0.0f);
}

// critic loss term of d = value - return and its derivative: mse or huber (delta 1)
MM_DEV void critic_term(float d, int huber, float &t_critic, float &dv) {
  if (huber) {
    const float ad = fabsf(d);
    t_critic = ad < 1.0f ? 0.5f * d * d : ad - 0.5f;
    dv = ad < 1.0f ? d : (d > 0.0f ? 1.0f : -1.0f);
  } else {
    t_critic = d * d;
    dv = 2.0f * d;
  }
}

// d loss / d logit[o] from g_lp = d loss / d logp_taken: g_lp (one_hot(act)[o] - softmax[o])
MM_DEV float dlogit(float g_lp, float logit, float lse, bool taken) { return g_lp * ((taken ? 1.0f : 0.0f) - expf(logit - lse)); }

// ---- dz1 = (W2^T dz2) . [h1 > 0]: a second MFMA contraction whose A operand is W2^T in fragment order.
// The forward's W2 fragments fill the LDS and a second copy for W2^T does not fit beside them; reading the transposed fragments
// out of the one staged copy puts the 64 lanes of a read on 8 banks (the lane's output row i only moves the address by (i & 3)
// floats and whole multiples of 128).  So the A operand comes from global memory: 16 float4 loads per lane and output tile from
// the fragment array `prep` wrote ([out tile][k chunk 4][group 4][lane 64] float4, L2 resident).
// w2t_fragment: element t of that array, for fc2 rows of `pitch` floats.
MM_DEV float4 w2t_fragment(const float *W2, int pitch, unsigned t) {
  const int l = t & 63, g = (t >> 6) & 3, m = (t >> 8) & 3, mt = t >> 10;
  const int i = l & 31, h = l >> 5;
  float w[4];
#pragma unroll
  for (int u = 0; u < 4; u++) w[u] = W2[(32 * m + frag_row(4 * g + u, h)) * pitch + 32 * mt + i];
  return make_float4(w[0], w[1], w[2], w[3]);
}

// The lane index made opaque once per tile: the fragment addresses (uniform base + one per-lane offset) are then formed where
// they are used instead of being hoisted out of the persistent loop into registers the kernel does not have.
MM_DEV unsigned opaque_lane(int lane) {
  unsigned vlane = (unsigned)lane;
  asm volatile("" : "+v"(vlane));
  return vlane;
}

// output tile mt of the contraction, before the ReLU mask of layer 1 (which the kernels apply from where they keep h1)
MM_DEV f32x16 dz1_tile(const float4 *frag, int mt, unsigned vlane, const f32x16 (&dz2)[4]) {
  f32x16 acc;
#pragma unroll
  for (int rr = 0; rr < 16; rr++) acc[rr] = 0.0f;
#pragma unroll
  for (int m = 0; m < 4; m++) {
#pragma unroll
    for (int g = 0; g < 4; g++)
      acc = mfma4((frag + ((mt * 4 + m) * 4 + g) * 64)[vlane], dz2[m][4 * g + 0], dz2[m][4 * g + 1], dz2[m][4 * g + 2],
                  dz2[m][4 * g + 3], acc);
  }
  return acc;
}

// ---- B = the number of valid samples (integer atomics: order-independent); thread t of a grid of 256-thread workgroups
MM_DEV void count_valid(const uint8_t *valid, long long n, int t, int *count) {
  if (valid) {
    int c = 0;
    for (long long k = t; k < n; k += (long long)gridDim.x * 256) c += valid[k] != 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
  } else if (t == 0) {
    *count = (int)n;
  }
}

// ---- the partial block one kernel-B workgroup writes, in floats, for a first layer of kL1 output tiles
template <int kL1>
struct PartialBlock {
  static constexpr int kW2 = 0;                           // [128][160]
  static constexpr int kHd = kW2 + kHidden * kW2Pitch;    // [16][128]: head rows (GI: 0..7 dWa, 8 dWc)
  static constexpr int kW1 = kHd + 16 * kHidden;          // [32 kL1][32]: dz1^T x, all columns
  static constexpr int kb2 = kW1 + 32 * kL1 * 32;         // [128]
  static constexpr int kbh = kb2 + kHidden;               // [16]
  static constexpr int kb1 = kbh + 16;                    // [32 kL1]
  static constexpr int kSize = kb1 + 32 * kL1;
};

// ---- kernel B: one workgroup (5 waves) = one slice of samples [row0, row1), whole 32-sample tiles inside n_pad; the sample index is the MFMA
// k dimension and both operands are coalesced row reads of the scratch.  h1 / dz1 have kL1 tiles (row pitch 32 kL1).  Wave w < 4
// owns output rows 32 w .. 32 w + 31 of dW2 = dz2^T [h1 | one_hot] (kL1 column tiles, + 1 with kOneHot: the one-hot row rebuilt
// from the action in column kActCol of the head row) and columns 32 w .. of the head tile dhead^T h2; wave 4 owns dW1 = dz1^T x.
// Bias sums on the VALU from the A operands, in fp64: one add per k-step, no rounding of a 10^3-term running sum.
// wgrad_rows: the contraction over rows [row0, row1) into the partial block `out`; wgrad_slice: workgroup b's slice of a batch.
template <int kL1, bool kOneHot>
MM_DEV void wgrad_rows(const float *s_h1, const float *s_dz1, const float *s_h2,
                       const float *s_dz2, const float *s_dh, const float *s_xs,
                       const long long row0, const long long row1, float *out) {
  typedef PartialBlock<kL1> P;
  constexpr int kPitch1 = 32 * kL1, kTiles2 = kL1 + (kOneHot ? 1 : 0);
  static_assert(32 * kTiles2 <= kW2Pitch, "dW2's column tiles fit a row of the partial");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, kh = lane >> 5;
  if (wave < 4) {
    const int mf = wave;
    f32x16 acc[kTiles2], acch;
#pragma unroll
    for (int c = 0; c < kTiles2; c++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[c][r] = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; r++) acch[r] = 0.0f;
    double bs2 = 0.0, bsh = 0.0;
    for (long long rb = row0 + kh; rb < row1; rb += 2 * kUnrollB)  // (a slice is a whole number of 32-sample tiles)
#pragma unroll
    for (int u = 0; u < kUnrollB; u++) {
      const long long row = rb + 2 * u;
      const float a2 = s_dz2[row * kHidden + 32 * mf + i];
      const float ah = i < kDh ? s_dh[row * kDh + i] : 0.0f;
      const float bh = s_h2[row * kHidden + 32 * mf + i];
      float b1[kTiles2];
#pragma unroll
      for (int c = 0; c < kL1; c++) b1[c] = s_h1[row * kPitch1 + 32 * c + i];
      if (kOneHot) b1[kTiles2 - 1] = (float)i == s_dh[row * kDh + kActCol] ? 1.0f : 0.0f;  // one_hot(action) row
#pragma unroll
      for (int c = 0; c < kTiles2; c++) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b1[c], acc[c], 0, 0, 0);
      acch = __builtin_amdgcn_mfma_f32_32x32x2f32(ah, bh, acch, 0, 0, 0);
      bs2 += (double)a2;
      bsh += (double)ah;
    }
    // accumulator register r of lane (j = i, h = kh): output row frag_row(r, kh), column j
#pragma unroll
    for (int c = 0; c < kTiles2; c++)
#pragma unroll
      for (int r = 0; r < 16; r++) out[P::kW2 + (32 * mf + frag_row(r, kh)) * kW2Pitch + 32 * c + i] = acc[c][r];
#pragma unroll
    for (int r = 0; r < 8; r++) out[P::kHd + frag_row(r, kh) * kHidden + 32 * mf + i] = acch[r];  // rows 0..15
    bs2 += __shfl_xor(bs2, 32, 64);
    bsh += __shfl_xor(bsh, 32, 64);
    if (kh == 0) {
      out[P::kb2 + 32 * mf + i] = (float)bs2;
      if (mf == 0 && i < kDh) out[P::kbh + i] = (float)bsh;
    }
  } else {
    f32x16 acc[kL1];
#pragma unroll
    for (int c = 0; c < kL1; c++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[c][r] = 0.0f;
    double bs1[kL1] = {};
    for (long long rb = row0 + kh; rb < row1; rb += 2 * kUnrollB)
#pragma unroll
    for (int u = 0; u < kUnrollB; u++) {
      const long long row = rb + 2 * u;
      const float bx = s_xs[row * kXs + i];
      float a1[kL1];
#pragma unroll
      for (int c = 0; c < kL1; c++) a1[c] = s_dz1[row * kPitch1 + 32 * c + i];
#pragma unroll
      for (int c = 0; c < kL1; c++) {
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[c], bx, acc[c], 0, 0, 0);
        bs1[c] += (double)a1[c];
      }
    }
#pragma unroll
    for (int c = 0; c < kL1; c++) {
#pragma unroll
      for (int r = 0; r < 16; r++) out[P::kW1 + (32 * c + frag_row(r, kh)) * 32 + i] = acc[c][r];
      const double s = bs1[c] + __shfl_xor(bs1[c], 32, 64);
      if (kh == 0) out[P::kb1 + 32 * c + i] = (float)s;
    }
  }
}

template <int kL1, bool kOneHot>
MM_DEV void wgrad_slice(const float *s_h1, const float *s_dz1, const float *s_h2,
                        const float *s_dz2, const float *s_dh, const float *s_xs,
                        long long n_pad, long long slice_rows, float *part) {
  const long long row0 = (long long)blockIdx.x * slice_rows;
  long long row1 = row0 + slice_rows;
  if (row1 > n_pad) row1 = n_pad;
  wgrad_rows<kL1, kOneHot>(s_h1, s_dz1, s_h2, s_dz2, s_dh, s_xs, row0, row1, part + (long long)blockIdx.x * PartialBlock<kL1>::kSize);
}

// ---- kernel C: element `off` of the partial blocks summed in workgroup order (fp64 running sum)
template <int kPartial>
MM_DEV float fold(const float *part, int slices, int off) {
  double s = 0.0;
#pragma unroll 8
  for (int g = 0; g < slices; g++) s += (double)part[(long long)g * kPartial + off];
  return (float)s;
}

// the per-tile loss partials (kSums interleaved per tile) folded by one 256-thread workgroup in a fixed tree into s[k][0]
template <int kSums>
MM_DEV void loss_tree(const double *lossp, long long ntiles, double (&s)[kSums][256]) {
  double p[kSums] = {};
  for (long long t = threadIdx.x; t < ntiles; t += 256) {
#pragma unroll
    for (int k = 0; k < kSums; k++) p[k] += lossp[kSums * t + k];
  }
#pragma unroll
  for (int k = 0; k < kSums; k++) s[k][threadIdx.x] = p[k];
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < kSums; k++) s[k][threadIdx.x] += s[k][threadIdx.x + o];
    }
    __syncthreads();
  }
}

MM_DEV double inv_count(const int *count) {
  const int nb = *count;
  return nb > 0 ? 1.0 / (double)nb : 0.0;
}

// ---- host side
// one persistent workgroup of `waves` waves per CU, fewer when there are fewer tiles
static unsigned persistent_grid(long long ntiles, int waves) {
  return (unsigned)(ntiles < waves * 256 ? (ntiles + waves - 1) / waves : 256);
}

// The scratch of a training call on n samples, offsets in floats: header, W2^T fragments, the per-sample rows of kernel A
// (h1, dz1 of pitch1 floats; h2, dz2; dhead; x), `sums` fp64 loss partials per tile, and one partial block of `partial` floats
// per kernel-B workgroup.  Kernel B's slices are whole 32-sample tiles, at least 2 tiles per slice.
struct Layout {
  long long n_pad, ntiles;
  long long frag, h1, dz1, h2, dz2, dh, xs, lossp, part, total;
  int slices;
  long long slice_rows;
};

static Layout scratch_layout(long long n, long long frag_floats, int pitch1, int sums, int partial) {
  Layout L;
  L.ntiles = (n + 31) / 32;
  L.n_pad = L.ntiles * 32;
  L.frag = kHdr;
  L.h1 = L.frag + frag_floats;
  L.dz1 = L.h1 + L.n_pad * pitch1;
  L.h2 = L.dz1 + L.n_pad * pitch1;
  L.dz2 = L.h2 + L.n_pad * kHidden;
  L.dh = L.dz2 + L.n_pad * kHidden;
  L.xs = L.dh + L.n_pad * kDh;
  L.lossp = L.xs + L.n_pad * kXs;  // double[ntiles][sums]
  L.part = L.lossp + 2 * sums * L.ntiles;
  const long long tiles_per = tiles_per_slice(L.ntiles);
  L.slices = (int)((L.ntiles + tiles_per - 1) / tiles_per);
  if (L.slices < 1) L.slices = 1;
  L.slice_rows = tiles_per * 32;
  L.total = L.part + (long long)L.slices * partial;
  return L;
}

// ---- what the training entries check alike, and their n == 0 path
static bool complete(const MMMlpParams *p) { return p && p->W1 && p->b1 && p->W2 && p->b2 && p->W3 && p->b3; }

static bool complete(const MMGiParams *p) {
  return p && p->W11 && p->b11 && p->W12 && p->b12 && p->W13 && p->b13 && p->W2 && p->b2 && p->Wa && p->ba && p->Wc && p->bc;
}

// `width`: the hidden size the entry is built for
static bool shape_ok(int64_t n, int32_t n_s, int32_t hidden, int32_t n_a, int32_t width) {
  return n >= 0 && n <= 0x7FFFFFFF && n_s >= 25 && n_s <= 32 && hidden == width && n_a >= 1 && n_a <= 8;
}

// a pass size: whole 32-sample tiles and kernel B's minimum of 2 tiles per slice
static bool chunk_ok(int64_t chunk) { return chunk > 0 && chunk % 64 == 0 && chunk <= 0x7FFFFFC0ll; }

template <typename T>
static T *shifted(T *p, long long by) { return p ? p + by : nullptr; }

// the gradient elements of a network with fc2 rows of k2 floats and n_out outputs: kernel C's threads
static int fold_elems(int hidden, int n_s, int k2, int n_out) { return hidden * n_s + hidden + hidden * k2 + hidden + n_out * hidden + n_out; }

// zeroes the six gradient tensors of `members` stacked networks of that shape; false: an enqueue failed
static bool zero_mlp_grads(hipStream_t s, const MMMlpParams *g, int hidden, int n_s, int k2, int n_out, int members = 1) {
  float *const gp[6] = {g->W1, g->b1, g->W2, g->b2, g->W3, g->b3};
  const size_t gsz[6] = {(size_t)hidden * n_s, (size_t)hidden, (size_t)hidden * k2, (size_t)hidden, (size_t)n_out * hidden, (size_t)n_out};
  for (int k = 0; k < 6; k++)
    if (hipMemsetAsync(gp[k], 0, gsz[k] * members * sizeof(float), s) != hipSuccess) return false;
  return true;
}

}  // namespace mfma
}  // namespace mm
#endif
