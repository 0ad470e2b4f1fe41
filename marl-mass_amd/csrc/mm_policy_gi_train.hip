// mm_policy_gi_train.hip -- loss and parameter gradient of MAPPO_GI's shared actor-critic (include/mm_policy_gi_train.h).
//
// The forward is policy_gi_kernel's (mm_policy_gi.hip), in the layout and from the pieces of mm_policy_mfma.h; the split gather
// of layer 1 is restated in kernel A, whose text is gi_sample_body of mm_policy_gi_sample.h, shared with the bank's training half
// (mm_policy_gi_bank_train.hip).
//
//   prep      W2^T in MFMA A-fragment order into the scratch (80 KB), and B = the number of valid samples.
//   kernel A  per sample: forward, heads, log-softmax, ratio, the loss terms, dlogit / dvalue (VALU tail);
//             dz2 = (Wa^T dlogit + Wc^T dvalue) . [h2 > 0] on the VALU (<= 9 rows, 64 features per lane);
//             dz1 = (W2^T dz2) . [h1 > 0] as a second 160 x 128 MFMA contraction (5 tiles x 64 k-steps; dz2 in accumulator
//             form is its B operand as h1 is the forward's), its A operand 80 float4 loads per lane and tile
//             from the 80 KB fragment array `prep` wrote (global, L2 resident: dz1_tile in mm_policy_mfma.h says why).
//             Stores h1, dz1 (160), h2, dz2 (128), dhead (16: dlogit 0..7, dvalue, zeros) and x (32: columns 0..24 of the
//             observation, zeros) per sample in [sample][feature] order, rows of masked / out-of-range samples as exact
//             zeros in every gradient row, and one (actor, critic) loss partial per 32 samples in fp64.
//   kernel B  contractions over the sample dimension, the sample index as the MFMA k dimension, both operands coalesced row
//             reads of the scratch: dW2 = dz2^T h1 (4 x 5 tiles), dhead^T h2 (4 tiles, rows 0..8 used), dz1^T x (5 tiles: all
//             25 columns, kernel C picks the block-diagonal ones of the split), bias sums on the VALU from the A operands.
//             5 waves per workgroup: wave w < 4 owns output rows 32 w .. 32 w + 31 of dW2 and columns of the head tile,
//             wave 4 the first layer.  Each workgroup contracts one contiguous slice of samples and writes one partial block.
//   kernel C  every parameter's gradient = the partial blocks summed in workgroup order (fp64 running sum), written in
//             torch layout; the loss partials folded by one workgroup in a fixed tree.
#include "mm_policy_chunked.h"  // PassArgs and the launch helpers' declarations; mm_policy_mfma.h and the public header
#include "mm_policy_gi_sample.h"  // kernel A

namespace mm {
namespace gi_train {

using namespace mfma;
constexpr int kCat = kGiCat;
constexpr int kThreadsA = kGiThreadsA;  // 8 waves = 2 per SIMD, as policy_gi_kernel
constexpr int kThreadsB = 320;  // 5 waves

constexpr long long kFrag = 5 * 4 * 4 * 64 * 4;  // W2^T fragments, in floats: [out tile 5][k chunk 4][group 4][lane 64] float4
typedef PartialBlock<5> Part;                    // the partial block of one kernel-B workgroup: 27 952 floats

static Layout layout(long long n) { return scratch_layout(n, kFrag, kCat, 2, Part::kSize); }

// ---- prep: W2^T fragments + the count of valid samples (integer atomics: order-independent)
__global__ __launch_bounds__(256) void gi_train_prep_kernel(const float *__restrict__ W2, float4 *__restrict__ frag,
                                                            const uint8_t *__restrict__ valid, long long n, int *__restrict__ count) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < 5 * 4 * 4 * 64) frag[t] = w2t_fragment(W2, kCat, t);
  count_valid(valid, n, t, count);
}

// ---- kernel A: gi_sample_body of mm_policy_gi_sample.h on the one network and the contiguous samples of the kernel's arguments
struct FlatArgs {
  const float *__restrict__ obs;
  long long obs_stride, n;
  const int32_t *__restrict__ actions;
  long long act_stride;
  const float *__restrict__ returns;
  long long ret_stride;
  const float *__restrict__ old_logp;
  const uint8_t *__restrict__ valid;
  MMGiParams w;
  int n_a;
  float clip_param;
  int huber;
  const float *__restrict__ adv_sums;
  const int *__restrict__ count;
  const float4 *__restrict__ frag;
  float *s_h1;
  float *__restrict__ s_dz1, *__restrict__ s_h2, *__restrict__ s_dz2, *__restrict__ s_dh, *__restrict__ s_xs;
  double *__restrict__ lossp;
  float *__restrict__ logp_out, *__restrict__ value_out, *__restrict__ ratio_out;
};

struct Flat {
  const FlatArgs &p;
  MM_DEV explicit Flat(const FlatArgs &a) : p(a) {}
  MM_DEV MMGiParams net() const { return p.w; }
  MM_DEV long long n() const { return p.n; }
  MM_DEV int count() const { return *p.count; }
  MM_DEV const float *adv_sums() const { return p.adv_sums; }
  MM_DEV bool ref_form() const { return p.adv_sums != nullptr; }
  MM_DEV const float4 *frag() const { return p.frag; }
  MM_DEV double *lossp() const { return p.lossp; }
  MM_DEV long long first_tile(int wave) const { return (long long)blockIdx.x * (kThreadsA / 64) + wave; }
  MM_DEV long long tile_stride() const { return (long long)gridDim.x * (kThreadsA / 64); }
  MM_DEV long long sample(long long i, bool) const { return i; }
  MM_DEV long long row(long long i) const { return i; }
};

__global__ __launch_bounds__(kThreadsA) void policy_gi_train_sample_kernel(
    const float *__restrict__ obs, long long obs_stride, long long n, const int32_t *__restrict__ actions, long long act_stride,
    const float *__restrict__ returns, long long ret_stride, const float *__restrict__ old_logp, const uint8_t *__restrict__ valid,
    MMGiParams w, int n_a, float clip_param, int huber, const float *__restrict__ adv_sums, const int *__restrict__ count,
    const float4 *__restrict__ frag, float *s_h1, float *__restrict__ s_dz1, float *__restrict__ s_h2,
    float *__restrict__ s_dz2, float *__restrict__ s_dh, float *__restrict__ s_xs, double *__restrict__ lossp,
    float *__restrict__ logp_out, float *__restrict__ value_out, float *__restrict__ ratio_out) {
  const FlatArgs a = {obs, obs_stride, n, actions, act_stride, returns, ret_stride, old_logp, valid, w, n_a, clip_param, huber, adv_sums,
                      count, frag, s_h1, s_dz1, s_h2, s_dz2, s_dh, s_xs, lossp, logp_out, value_out, ratio_out};
  gi_sample_body<true>(Flat(a));
}

// ---- kernel B: one workgroup = one slice of samples [row0, row1), rows are whole 32-sample tiles inside n_pad
__global__ __launch_bounds__(kThreadsB) void policy_gi_train_wgrad_kernel(
    const float *__restrict__ s_h1, const float *__restrict__ s_dz1, const float *__restrict__ s_h2, const float *__restrict__ s_dz2,
    const float *__restrict__ s_dh, const float *__restrict__ s_xs, long long n_pad, long long slice_rows, float *__restrict__ part) {
  wgrad_slice<5, false>(s_h1, s_dz1, s_h2, s_dz2, s_dh, s_xs, n_pad, slice_rows, part);
}

// ---- kernel C: gradient element t = sum over the partial blocks in workgroup order; the last workgroup folds the losses
constexpr int kNFixed = 32 * 5 + 32 + 64 * 10 + 64 + 64 * 10 + 64 + kHidden * kCat + kHidden;  // everything before Wa

MM_DEV float fold(const float *__restrict__ part, int slices, int off) { return mfma::fold<Part::kSize>(part, slices, off); }

__global__ __launch_bounds__(256) void policy_gi_train_fold_kernel(const float *__restrict__ part, int slices, int n_a, MMGiParams gr,
                                                                   const double *__restrict__ lossp, long long ntiles,
                                                                   const int *__restrict__ count, int ref_form,
                                                                   float *__restrict__ loss) {
  const int nelem = kNFixed + n_a * kHidden + n_a + kHidden + 1;
  if (blockIdx.x == gridDim.x - 1) {
    __shared__ double ssum[2][256];  // actor, critic
    loss_tree<2>(lossp, ntiles, ssum);
    if (threadIdx.x == 0) {
      const double inv = inv_count(count);
      const float a = (float)(-ssum[0][0] * inv * (ref_form ? inv : 1.0)), c = (float)(ssum[1][0] * inv);
      loss[0] = a;
      loss[1] = c;
      loss[2] = a + c;
    }
    return;
  }
  int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nelem) return;
  if (t < 160) { const int o = t / 5, k = t % 5; gr.W11[t] = fold(part, slices, Part::kW1 + o * 32 + 5 * k); return; }
  t -= 160;
  if (t < 32) { gr.b11[t] = fold(part, slices, Part::kb1 + t); return; }
  t -= 32;
  if (t < 640) { const int o = t / 10, k = t % 10; gr.W12[t] = fold(part, slices, Part::kW1 + (32 + o) * 32 + 5 * (k >> 1) + 1 + (k & 1)); return; }
  t -= 640;
  if (t < 64) { gr.b12[t] = fold(part, slices, Part::kb1 + 32 + t); return; }
  t -= 64;
  if (t < 640) { const int o = t / 10, k = t % 10; gr.W13[t] = fold(part, slices, Part::kW1 + (96 + o) * 32 + 5 * (k >> 1) + 3 + (k & 1)); return; }
  t -= 640;
  if (t < 64) { gr.b13[t] = fold(part, slices, Part::kb1 + 96 + t); return; }
  t -= 64;
  if (t < kHidden * kCat) { gr.W2[t] = fold(part, slices, Part::kW2 + t); return; }
  t -= kHidden * kCat;
  if (t < kHidden) { gr.b2[t] = fold(part, slices, Part::kb2 + t); return; }
  t -= kHidden;
  if (t < n_a * kHidden) { gr.Wa[t] = fold(part, slices, Part::kHd + t); return; }
  t -= n_a * kHidden;
  if (t < n_a) { gr.ba[t] = fold(part, slices, Part::kbh + t); return; }
  t -= n_a;
  if (t < kHidden) { gr.Wc[t] = fold(part, slices, Part::kHd + 8 * kHidden + t); return; }
  gr.bc[0] = fold(part, slices, Part::kbh + 8);
}

// ---- host-side launch helpers (declared in mm_policy_chunked.h): the one spelling of each launch, on the samples and rows the
// caller points at -- the whole batch for the entry below, one pass for the pass loops of mm_policy_chunked.hip
Layout layout_of(long long n) { return layout(n); }

void launch_prep(hipStream_t s, const float *W2, float4 *frag, const uint8_t *valid, long long n, int *count) {
  hipLaunchKernelGGL(gi_train_prep_kernel, dim3(5 * 4 * 4 * 64 / 256), dim3(256), 0, s, W2, frag, valid, n, count);
}

void launch_sample(hipStream_t s, const PassArgs &p) {
  const unsigned gridA = persistent_grid((p.n + 31) / 32, kThreadsA / 64);
  hipLaunchKernelGGL(policy_gi_train_sample_kernel, dim3(gridA), dim3(kThreadsA), 0, s, p.obs, p.obs_stride, p.n, p.actions,
                     p.act_stride, p.returns, p.ret_stride, p.old_logp, p.valid, p.w, p.n_a, p.clip_param, p.huber, p.adv_sums,
                     p.count, p.frag, p.rows.h1, p.rows.dz1, p.rows.h2, p.rows.dz2, p.rows.dh, p.rows.xs, p.lossp, p.logp_out,
                     p.value_out, p.ratio_out);
}

void launch_wgrad(hipStream_t s, const SampleRows &r, long long n_pad, long long slice_rows, int slices, float *part) {
  hipLaunchKernelGGL(policy_gi_train_wgrad_kernel, dim3(slices), dim3(kThreadsB), 0, s, r.h1, r.dz1, r.h2, r.dz2, r.dh, r.xs, n_pad,
                     slice_rows, part);
}

bool zero_grads(hipStream_t s, const MMGiParams &g, int n_a) {
  float *const gp[12] = {g.W11, g.b11, g.W12, g.b12, g.W13, g.b13, g.W2, g.b2, g.Wa, g.ba, g.Wc, g.bc};
  const size_t gsz[12] = {160, 32, 640, 64, 640, 64, (size_t)kHidden * kCat, kHidden, (size_t)n_a * kHidden, (size_t)n_a, kHidden, 1};
  for (int k = 0; k < 12; k++)
    if (hipMemsetAsync(gp[k], 0, gsz[k] * sizeof(float), s) != hipSuccess) return false;
  return true;
}

}  // namespace gi_train
}  // namespace mm

extern "C" int32_t mm_policy_gi_train_scratch_bytes(int64_t n, uint64_t *bytes) {
  if (n < 0 || !bytes) return MM_ERR_INVALID_ARG;
  *bytes = (uint64_t)mm::gi_train::layout(n).total * 4u;
  return MM_OK;
}

extern "C" int32_t mm_policy_gi_train(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                      int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                      const uint8_t *valid, const MMGiParams *weights, int32_t hidden, int32_t n_a,
                                      float clip_param, int32_t critic_loss, const float *adv_sums, const MMGiParams *grads,
                                      float *loss, float *logp_taken, float *value, float *ratio, void *scratch,
                                      uint64_t scratch_bytes, MMStream stream) {
  using namespace mm::gi_train;
  if (!complete(weights) || !complete(grads) || !loss || !shape_ok(n, n_s, hidden, n_a, kHidden)) return MM_ERR_INVALID_ARG;
  if (critic_loss != MM_GI_CRITIC_MSE && critic_loss != MM_GI_CRITIC_HUBER) return MM_ERR_INVALID_ARG;
  if (!(clip_param >= 0.0f)) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (!zero_grads(s, *grads, n_a) || hipMemsetAsync(loss, 0, 3 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
    return MM_OK;
  }
  if (!obs || !actions || !returns || !old_logp || obs_stride < n_s) return MM_ERR_INVALID_ARG;
  const Layout L = layout(n);
  if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < (uint64_t)L.total * 4u) return MM_ERR_INVALID_ARG;
  float *sc = (float *)scratch;
  int *count = (int *)sc;
  if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess) return MM_ERR_DEVICE;
  PassArgs p = {};  // the whole batch in one pass
  p.obs = obs; p.obs_stride = obs_stride; p.n = n; p.actions = actions; p.act_stride = act_stride; p.returns = returns;
  p.ret_stride = ret_stride; p.old_logp = old_logp; p.valid = valid; p.w = *weights; p.n_a = n_a; p.clip_param = clip_param;
  p.huber = critic_loss == MM_GI_CRITIC_HUBER; p.adv_sums = adv_sums; p.count = count;
  p.frag = (const float4 *)(sc + L.frag); p.rows = mm::chunked::rows_of(sc, L); p.lossp = (double *)(sc + L.lossp);
  p.logp_out = logp_taken; p.value_out = value; p.ratio_out = ratio;
  launch_prep(s, p.w.W2, (float4 *)(sc + L.frag), valid, n, count);
  launch_sample(s, p);
  launch_wgrad(s, p.rows, L.n_pad, L.slice_rows, L.slices, sc + L.part);
  const int nelem = kNFixed + n_a * kHidden + n_a + kHidden + 1;
  hipLaunchKernelGGL(policy_gi_train_fold_kernel, dim3((nelem + 255) / 256 + 1), dim3(256), 0, s, sc + L.part, L.slices, (int)n_a,
                     *grads, (const double *)p.lossp, L.ntiles, (const int *)count, (int)(adv_sums != nullptr), loss);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
