// mm_policy_chunked.hip -- the gradient of a whole batch under a fixed scratch budget: mm_policy_gi_train_chunked
// (include/mm_policy_gi_train.h) and mm_policy_train_chunked (include/mm_policy_train.h).
//
// The unchunked entries keep every sample's activations between kernel A and kernel B (2 496 B / 2 240 B per sample).  Here
// kernels A and B -- the SAME kernels, launched through the host helpers of mm_policy_chunked.h -- run over the batch in passes
// of `chunk` samples through one set of per-sample rows, and what kernel C folds in one go is folded across the passes:
//
//   memset     the fp64 accumulator block(s) and the count
//   prep       once, over the whole batch: the W2^T fragments and B = the number of valid samples of ALL n (kernel A scales by it)
//   per pass   kernel A on samples [c chunk, min(n, (c + 1) chunk)) (the per-sample pointers offset on the host, the loss
//              partials at the pass's first tile of the global array), kernel B on the pass's slices, then
//              accumulate: acc[off] += the pass's partial blocks in workgroup order, fp64
//   finish     acc -> float in torch layout (the index maps of the two fold kernels); one more workgroup folds the loss partials
//              of all ceil(n / 32) tiles with the same tree and count as the unchunked fold.
//
// A gradient element is float(the fp64 running sum of all partial blocks of all passes, in pass and workgroup order): exactly
// what the unchunked fold computes over its one pass, so chunk >= n gives the unchunked entry's bits.  Losses and diagnostics are
// per tile / per sample and do not depend on the slicing at all.  No floating-point atomics; only enqueues on the stream.
//
// chunk is a positive multiple of 64: every pass but the last is whole 32-sample tiles (the loss partials and the diagnostics
// of a pass start on a tile boundary of the global arrays) and a slice of kernel B keeps its minimum of 2 tiles.
#include "mm_policy_chunked.h"

namespace mm {
namespace chunked {

using namespace mfma;

// ---- accumulate: one thread per partial-block element; consecutive threads read consecutive floats of a block.
// It walks the whole block, the elements no kernel B writes included (the actor's one-hot tile of dW2: columns 128..159 of its
// 160-float rows): what lands in their accumulator slots is whatever the scratch held, and finish never reads those slots.
__global__ __launch_bounds__(256) void train_chunked_accumulate_kernel(const float *__restrict__ part, int slices, int size,
                                                                       double *__restrict__ acc) {
  const int off = blockIdx.x * 256 + threadIdx.x;
  if (off >= size) return;
  double s = acc[off];
#pragma unroll 8
  for (int g = 0; g < slices; g++) s += (double)part[(long long)g * size + off];
  acc[off] = s;
}

// ---- finish, shared network: gi_grad_slot's index map (mm_policy_chunked.h) on the accumulator
__global__ __launch_bounds__(256) void policy_gi_train_chunked_finish_kernel(const double *__restrict__ acc, int n_a, MMGiParams gr,
                                                                             const double *__restrict__ lossp, long long ntiles,
                                                                             const int *__restrict__ count, int ref_form,
                                                                             float *__restrict__ loss) {
  const int nelem = gi_elems(n_a);
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
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nelem) return;
  int src;
  float *dst = gi_grad_slot(t, n_a, gr, src);
  *dst = (float)acc[src];
}

// ---- finish, one separate network: pt_grad_slot's index map (mm_policy_chunked.h) on the accumulator
// loss_mode 0: sum / B (critic); 1: -sum / B (actor, per-sample form); 2: -sum / B^2 (actor, reference form)
__global__ __launch_bounds__(256) void policy_train_chunked_finish_kernel(const double *__restrict__ acc, int n_s, int k2, int n_out,
                                                                          MMMlpParams gr, const double *__restrict__ lossp,
                                                                          long long ntiles, const int *__restrict__ count,
                                                                          int loss_mode, float *__restrict__ loss) {
  if (blockIdx.x == gridDim.x - 1) {
    __shared__ double ssum[1][256];
    loss_tree<1>(lossp, ntiles, ssum);
    if (threadIdx.x == 0) {
      const double inv = inv_count(count);
      *loss = (float)(loss_mode == 0 ? ssum[0][0] * inv : (loss_mode == 1 ? -ssum[0][0] * inv : -ssum[0][0] * inv * inv));
    }
    return;
  }
  int src;
  float *dst = pt_grad_slot(blockIdx.x * 256 + threadIdx.x, n_s, k2, n_out, gr, src);
  if (dst) *dst = (float)acc[src];
}

// ---- host side (the scratch layout: mm_policy_chunked.h)
void accumulate(hipStream_t s, const float *part, int slices, int size, double *acc) {
  hipLaunchKernelGGL(train_chunked_accumulate_kernel, dim3((size + 255) / 256), dim3(256), 0, s, part, slices, size, acc);
}

}  // namespace chunked
}  // namespace mm

extern "C" int32_t mm_policy_gi_train_chunked_scratch_bytes(int64_t n, int64_t chunk, uint64_t *bytes) {
  using namespace mm::chunked;
  if (n < 0 || n > 0x7FFFFFFF || !chunk_ok(chunk) || !bytes) return MM_ERR_INVALID_ARG;
  *bytes = (uint64_t)chunk_layout(mm::gi_train::layout_of(chunk), n, 2, PartGi::kSize, 1).total * 4u;
  return MM_OK;
}

extern "C" int32_t mm_policy_gi_train_chunked(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                              int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                              const uint8_t *valid, const MMGiParams *weights, int32_t hidden, int32_t n_a,
                                              float clip_param, int32_t critic_loss, const float *adv_sums, const MMGiParams *grads,
                                              float *loss, float *logp_taken, float *value, float *ratio, void *scratch,
                                              uint64_t scratch_bytes, MMStream stream, int64_t chunk) {
  using namespace mm::chunked;
  namespace gi = mm::gi_train;
  if (!weights || !grads || !loss) return MM_ERR_INVALID_ARG;
  const MMGiParams W = *weights, G = *grads;  // (passed to the kernels by value)
  float *const wp[12] = {W.W11, W.b11, W.W12, W.b12, W.W13, W.b13, W.W2, W.b2, W.Wa, W.ba, W.Wc, W.bc};
  float *const gp[12] = {G.W11, G.b11, G.W12, G.b12, G.W13, G.b13, G.W2, G.b2, G.Wa, G.ba, G.Wc, G.bc};
  for (int k = 0; k < 12; k++)
    if (!wp[k] || !gp[k]) return MM_ERR_INVALID_ARG;
  if (n < 0 || n > 0x7FFFFFFF || n_s < 25 || n_s > 32 || hidden != kHidden || n_a < 1 || n_a > 8) return MM_ERR_INVALID_ARG;
  if (critic_loss != MM_GI_CRITIC_MSE && critic_loss != MM_GI_CRITIC_HUBER) return MM_ERR_INVALID_ARG;
  if (!(clip_param >= 0.0f) || !chunk_ok(chunk)) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t gsz[12] = {160, 32, 640, 64, 640, 64, (size_t)kHidden * kCatGi, kHidden, (size_t)n_a * kHidden, (size_t)n_a, kHidden, 1};
  if (n == 0) {
    for (int k = 0; k < 12; k++)
      if (hipMemsetAsync(gp[k], 0, gsz[k] * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
    if (hipMemsetAsync(loss, 0, 3 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
    return MM_OK;
  }
  if (!obs || !actions || !returns || !old_logp || obs_stride < n_s) return MM_ERR_INVALID_ARG;
  const ChunkLayout L = chunk_layout(gi::layout_of(chunk), n, 2, PartGi::kSize, 1);
  if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < (uint64_t)L.total * 4u) return MM_ERR_INVALID_ARG;
  const long long last = n % chunk ? n % chunk : (long long)chunk;  // the two pass sizes there are: chunk and the last pass's
  if (gi::layout_of(n < chunk ? n : chunk).slices > L.blocks || gi::layout_of(last).slices > L.blocks) return MM_ERR_INVALID_ARG;
  float *sc = (float *)scratch;
  int *count = (int *)sc;
  double *acc = (double *)(sc + L.acc), *lossp = (double *)(sc + L.lossp);
  if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess) return MM_ERR_DEVICE;
  if (hipMemsetAsync(acc, 0, PartGi::kSize * sizeof(double), s) != hipSuccess) return MM_ERR_DEVICE;
  gi::launch_prep(s, W.W2, (float4 *)(sc + L.rows.frag), valid, (long long)n, count);
  gi::PassArgs p = {};
  p.obs_stride = obs_stride; p.act_stride = act_stride; p.ret_stride = ret_stride; p.w = W; p.n_a = n_a; p.clip_param = clip_param;
  p.huber = critic_loss == MM_GI_CRITIC_HUBER; p.adv_sums = adv_sums; p.count = count;
  p.frag = (const float4 *)(sc + L.rows.frag); p.rows = rows_of(sc, L.rows);
  for (long long c0 = 0; c0 < n; c0 += chunk) {
    const long long np = n - c0 < chunk ? n - c0 : (long long)chunk;
    const Layout P = gi::layout_of(np);  // the pass's tiles and slices
    p.n = np;
    p.obs = obs + c0 * obs_stride; p.actions = actions + c0 * act_stride; p.returns = returns + c0 * ret_stride;
    p.old_logp = old_logp + c0; p.valid = shifted(valid, c0);
    p.lossp = lossp + 2 * (c0 / 32);
    p.logp_out = shifted(logp_taken, c0); p.value_out = shifted(value, c0); p.ratio_out = shifted(ratio, c0);
    gi::launch_sample(s, p);
    gi::launch_wgrad(s, p.rows, P.n_pad, P.slice_rows, P.slices, sc + L.part);
    accumulate(s, sc + L.part, P.slices, PartGi::kSize, acc);
  }
  const int nelem = gi_elems(n_a);
  hipLaunchKernelGGL(policy_gi_train_chunked_finish_kernel, dim3((nelem + 255) / 256 + 1), dim3(256), 0, s, (const double *)acc,
                     (int)n_a, G, (const double *)lossp, L.ntiles, (const int *)count, (int)(adv_sums != nullptr), loss);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

extern "C" int32_t mm_policy_train_chunked_scratch_bytes(int64_t n, int64_t chunk, uint64_t *bytes) {
  using namespace mm::chunked;
  if (n < 0 || n > 0x7FFFFFFF || !chunk_ok(chunk) || !bytes) return MM_ERR_INVALID_ARG;
  *bytes = (uint64_t)chunk_layout(mm::pt::layout_of(chunk), n, 2, PartPt::kSize, 2).total * 4u;
  return MM_OK;
}

static bool pt_complete(const MMMlpParams *p) { return p && p->W1 && p->b1 && p->W2 && p->b2 && p->W3 && p->b3; }

extern "C" int32_t mm_policy_train_chunked(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                           int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                           const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden,
                                           int32_t n_a, float clip_param, int32_t critic_loss, const float *adv_sums,
                                           const float *advantages, const MMMlpParams *actor_grads, const MMMlpParams *critic_grads,
                                           float *loss, float *logp_taken, float *value, float *ratio, void *scratch,
                                           uint64_t scratch_bytes, MMStream stream, int64_t chunk) {
  using namespace mm::chunked;
  namespace pt = mm::pt;
  if ((!actor && !critic) || !loss) return MM_ERR_INVALID_ARG;
  if ((actor != nullptr) != (actor_grads != nullptr) || (critic != nullptr) != (critic_grads != nullptr)) return MM_ERR_INVALID_ARG;
  if ((actor && (!pt_complete(actor) || !pt_complete(actor_grads))) || (critic && (!pt_complete(critic) || !pt_complete(critic_grads))))
    return MM_ERR_INVALID_ARG;
  if (n < 0 || n > 0x7FFFFFFF || n_s < 25 || n_s > 32 || hidden != kHidden || n_a < 1 || n_a > 8) return MM_ERR_INVALID_ARG;
  if (critic_loss != MM_PT_CRITIC_MSE && critic_loss != MM_PT_CRITIC_HUBER) return MM_ERR_INVALID_ARG;
  if (!(clip_param >= 0.0f) || !chunk_ok(chunk)) return MM_ERR_INVALID_ARG;
  if ((!actor && (logp_taken || ratio)) || (!critic && value)) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int k2c = kHidden + n_a;
  // everything that can refuse the call comes before the first enqueue
  ChunkLayout L = {};
  if (n > 0) {
    if (!obs || !actions || obs_stride < n_s || (actor && !old_logp) || (critic && !returns)) return MM_ERR_INVALID_ARG;
    if (actor && ((adv_sums != nullptr) == (advantages != nullptr))) return MM_ERR_INVALID_ARG;
    // the two networks' loss partials live side by side: both are folded at the end, after the passes alternated over the rows
    L = chunk_layout(pt::layout_of(chunk), n, 2, PartPt::kSize, 2);
    if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < (uint64_t)L.total * 4u) return MM_ERR_INVALID_ARG;
    const long long last = n % chunk ? n % chunk : (long long)chunk;
    if (pt::layout_of(n < chunk ? n : chunk).slices > L.blocks || pt::layout_of(last).slices > L.blocks) return MM_ERR_INVALID_ARG;
  }
  if (hipMemsetAsync(loss, 0, 2 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
  if (n == 0) {
    for (int net = 0; net < 2; net++) {
      const MMMlpParams *g = net ? critic_grads : actor_grads;
      if (!g) continue;
      const int k2 = net ? k2c : kHidden, n_out = net ? 1 : n_a;
      float *const gp[6] = {g->W1, g->b1, g->W2, g->b2, g->W3, g->b3};
      const size_t gsz[6] = {(size_t)kHidden * n_s, kHidden, (size_t)kHidden * k2, kHidden, (size_t)n_out * kHidden, (size_t)n_out};
      for (int k = 0; k < 6; k++)
        if (hipMemsetAsync(gp[k], 0, gsz[k] * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
    }
    return MM_OK;
  }
  float *sc = (float *)scratch;
  int *count = (int *)sc;
  double *acc_a = (double *)(sc + L.acc), *acc_c = acc_a + PartPt::kSize;
  double *lossp_a = (double *)(sc + L.lossp), *lossp_c = lossp_a + L.ntiles;
  if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess) return MM_ERR_DEVICE;
  if (hipMemsetAsync(acc_a, 0, 2 * PartPt::kSize * sizeof(double), s) != hipSuccess) return MM_ERR_DEVICE;
  pt::launch_prep(s, actor ? actor->W2 : nullptr, critic ? critic->W2 : nullptr, k2c, (float4 *)(sc + L.rows.frag), valid, (long long)n,
                  count);
  pt::PassArgs p = {};
  p.obs_stride = obs_stride; p.n_s = n_s; p.act_stride = act_stride; p.ret_stride = ret_stride; p.n_a = n_a;
  p.clip_param = clip_param; p.huber = critic_loss == MM_PT_CRITIC_HUBER; p.adv_sums = adv_sums; p.count = count;
  p.rows = rows_of(sc, L.rows);
  for (long long c0 = 0; c0 < n; c0 += chunk) {
    const long long np = n - c0 < chunk ? n - c0 : (long long)chunk;
    const Layout P = pt::layout_of(np);  // the pass's tiles and slices
    p.n = np;
    p.obs = obs + c0 * obs_stride; p.actions = actions + c0 * act_stride; p.returns = shifted(returns, c0 * ret_stride);
    p.old_logp = shifted(old_logp, c0); p.valid = shifted(valid, c0); p.advantages = shifted(advantages, c0);
    if (actor) {
      p.w = *actor; p.frag = (const float4 *)(sc + L.rows.frag); p.lossp = lossp_a + c0 / 32;
      p.out0 = shifted(logp_taken, c0); p.out1 = shifted(ratio, c0);
      pt::launch_sample(s, false, p);
      pt::launch_wgrad(s, false, p.rows, P.n_pad, P.slice_rows, P.slices, sc + L.part);
      accumulate(s, sc + L.part, P.slices, PartPt::kSize, acc_a);
    }
    if (critic) {
      p.w = *critic; p.frag = (const float4 *)(sc + L.rows.frag + pt::critic_frag_offset()); p.lossp = lossp_c + c0 / 32;
      p.out0 = shifted(value, c0); p.out1 = nullptr;
      pt::launch_sample(s, true, p);
      pt::launch_wgrad(s, true, p.rows, P.n_pad, P.slice_rows, P.slices, sc + L.part);
      accumulate(s, sc + L.part, P.slices, PartPt::kSize, acc_c);
    }
  }
  if (actor)
    hipLaunchKernelGGL(policy_train_chunked_finish_kernel, dim3((pt_elems(n_s, kHidden, n_a) + 255) / 256 + 1), dim3(256), 0, s,
                       (const double *)acc_a, (int)n_s, kHidden, (int)n_a, *actor_grads, (const double *)lossp_a, L.ntiles,
                       (const int *)count, adv_sums ? 2 : 1, loss);
  if (critic)
    hipLaunchKernelGGL(policy_train_chunked_finish_kernel, dim3((pt_elems(n_s, k2c, 1) + 255) / 256 + 1), dim3(256), 0, s,
                       (const double *)acc_c, (int)n_s, k2c, 1, *critic_grads, (const double *)lossp_c, L.ntiles, (const int *)count, 0,
                       loss + 1);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
