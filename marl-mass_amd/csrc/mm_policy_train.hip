// mm_policy_train.hip -- loss and parameter gradient of MAPPO's separate actor and critic (include/mm_policy_train.h), and the
// forward-only mm_policy_eval.
//
// The shape is mm_policy_gi_train.hip's, in the layout and from the pieces of mm_policy_mfma.h.
//
//   prep      W2[:, :128]^T of each given network in MFMA A-fragment order into the scratch (64 KB each), and B = the number
//             of valid samples.
//   kernel A  mlp_sample_kernel of mm_policy_sample.h, on the one network and the contiguous samples of a call (`Flat`).
//   kernel B  contractions over the sample dimension, the sample index as the MFMA k dimension, both operands coalesced row
//             reads of the scratch: dW2 = dz2^T [h1 | one_hot] (4 x 4 or 4 x 5 tiles), dW3 = dhead^T h2 (4 tiles), dW1 =
//             dz1^T x (4 tiles), bias sums on the VALU from the A operands.  5 waves per workgroup: wave w < 4 owns output
//             rows 32 w .. 32 w + 31 of dW2 and columns of the head tile, wave 4 the first layer.  Each workgroup contracts one
//             contiguous slice of samples and writes one partial block.
//   kernel C  every parameter's gradient = the partial blocks summed in workgroup order (fp64 running sum), written in
//             torch layout; the loss partials folded by one workgroup in a fixed tree.
// The actor's three kernels run first, then the critic's over the same scratch (stream order).
#include "mm_policy_chunked.h"  // PassArgs and the launch helpers' declarations; mm_policy_mfma.h and the public header
#include "mm_policy_sample.h"   // kernel A

namespace mm {
namespace pt {

using namespace mfma;
constexpr int kCat = kW2Pitch;  // row pitch of the dW2 partial: 128 + the one-hot tile
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

// ---- kernel A: mlp_sample_kernel of mm_policy_sample.h on the one network and the contiguous samples of a SampleArgs
struct Flat {
  const SampleArgs &p;
  MM_DEV explicit Flat(const SampleArgs &a) : p(a) {}
  MM_DEV long long n() const { return p.n; }
  MM_DEV MMMlpParams net(int, int, int) const { return p.w; }
  MM_DEV int count() const { return *p.count; }
  MM_DEV const float *adv_sums() const { return p.adv_sums; }
  MM_DEV bool ref_form() const { return p.adv_sums != nullptr; }
  MM_DEV const float4 *frag() const { return p.frag; }
  MM_DEV double *lossp() const { return p.lossp; }
  MM_DEV long long first_tile(int wave) const { return (long long)blockIdx.x * (kThreadsA / 64) + wave; }
  MM_DEV long long tile_stride() const { return (long long)gridDim.x * (kThreadsA / 64); }
  MM_DEV long long sample(long long i, bool) const { return i; }
  MM_DEV long long row(long long i) const { return i; }
  MM_DEV float advantage(long long ag) const { return p.advantages[ag]; }
};

template <bool kCritic, bool kTrain>
constexpr auto policy_train_sample_kernel = mlp_sample_kernel<kCritic, kTrain, Flat, SampleArgs>;

// ---- kernel B: one workgroup = one slice of samples [row0, row1), rows are whole 32-sample tiles inside n_pad
template <bool kCritic>
__global__ __launch_bounds__(kThreadsB) void policy_train_wgrad_kernel(
    const float *__restrict__ s_h1, const float *__restrict__ s_dz1, const float *__restrict__ s_h2, const float *__restrict__ s_dz2,
    const float *__restrict__ s_dh, const float *__restrict__ s_xs, long long n_pad, long long slice_rows, float *__restrict__ part) {
  wgrad_slice<4, kCritic>(s_h1, s_dz1, s_h2, s_dz2, s_dh, s_xs, n_pad, slice_rows, part);
}

// ---- kernel C: gradient element t = sum over the partial blocks in workgroup order; the last workgroup folds the loss
MM_DEV float fold(const float *__restrict__ part, int slices, int off) { return mfma::fold<Part::kSize>(part, slices, off); }

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
  hipLaunchKernelGGL((critic ? policy_train_sample_kernel<true, true> : policy_train_sample_kernel<false, true>), dim3(grid),
                     dim3(kThreadsA), 0, s, a);
}

void launch_wgrad(hipStream_t s, bool critic, const SampleRows &r, long long n_pad, long long slice_rows, int slices, float *part) {
  hipLaunchKernelGGL((critic ? policy_train_wgrad_kernel<true> : policy_train_wgrad_kernel<false>), dim3(slices), dim3(kThreadsB), 0,
                     s, r.h1, r.dz1, r.h2, r.dz2, r.dh, r.xs, n_pad, slice_rows, part);
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
    hipLaunchKernelGGL(policy_train_fold_kernel, dim3((fold_elems(kHidden, n_s, k2, n_out) + 255) / 256 + 1), dim3(256), 0, s, sc + L.part,
                       L.slices, (int)n_s, k2, n_out, net ? *critic_grads : *actor_grads, (const double *)p.lossp, L.ntiles,
                       (const int *)count, net ? 0 : (adv_sums ? 2 : 1), loss + net);
  }
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
