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

// ---- host side (the scratch layout: mm_policy_chunked.h): the accumulate launch, then each family's argument check and pass
// loop, which the entries below run on the whole batch and the rank-sharded ones (mm_policy_sharded.hip) on a rank's samples
void accumulate(hipStream_t s, const float *part, int slices, int size, double *acc) {
  hipLaunchKernelGGL(train_chunked_accumulate_kernel, dim3((size + 255) / 256), dim3(256), 0, s, part, slices, size, acc);
}

static bool scratch_ok(const ChunkLayout &L, Layout (*layout_of)(long long), long long n, long long chunk, const void *scratch,
                       uint64_t scratch_bytes) {
  if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < (uint64_t)L.total * 4u) return false;
  const long long last = n % chunk ? n % chunk : chunk;  // the two pass sizes there are: chunk and the last pass's
  return layout_of(n < chunk ? n : chunk).slices <= L.blocks && layout_of(last).slices <= L.blocks;
}

bool gi_args_ok(const gi_train::PassArgs &b, int32_t n_s, int32_t hidden, int32_t critic_loss, int64_t chunk, const void *scratch,
                uint64_t scratch_bytes, ChunkLayout &L) {
  L = {};
  if (!complete(&b.w) || !shape_ok(b.n, n_s, hidden, b.n_a, kHidden)) return false;
  if (critic_loss != MM_GI_CRITIC_MSE && critic_loss != MM_GI_CRITIC_HUBER) return false;
  if (!(b.clip_param >= 0.0f) || !chunk_ok(chunk)) return false;
  if (b.n == 0) return true;  // (empty inputs and the scratch are not looked at and may be NULL)
  if (!b.obs || !b.actions || !b.returns || !b.old_logp || b.obs_stride < n_s) return false;
  L = chunk_layout(gi_train::layout_of(chunk), b.n, 2, PartGi::kSize, 1);
  return scratch_ok(L, gi_train::layout_of, b.n, chunk, scratch, scratch_bytes);
}

bool pt_args_ok(const pt::PassArgs &b, const PtNet (&net)[2], int32_t hidden, int32_t critic_loss, int64_t chunk, const void *scratch,
                uint64_t scratch_bytes, ChunkLayout &L) {
  L = {};
  const bool actor = net[0].w != nullptr, critic = net[1].w != nullptr;
  if ((!actor && !critic) || (actor && !complete(net[0].w)) || (critic && !complete(net[1].w))) return false;
  if (!shape_ok(b.n, b.n_s, hidden, b.n_a, kHidden)) return false;
  if (critic_loss != MM_PT_CRITIC_MSE && critic_loss != MM_PT_CRITIC_HUBER) return false;
  if (!(b.clip_param >= 0.0f) || !chunk_ok(chunk)) return false;
  if ((!actor && (net[0].out0 || net[0].out1)) || (!critic && net[1].out0)) return false;
  if (b.n == 0) return true;  // (empty inputs, adv_sums, advantages and the scratch are not looked at and may be NULL)
  if (!b.obs || !b.actions || b.obs_stride < b.n_s || (actor && !b.old_logp) || (critic && !b.returns)) return false;
  if (actor && ((b.adv_sums != nullptr) == (b.advantages != nullptr))) return false;
  // the two networks' loss partials live side by side: both are folded at the end, after the passes alternated over the rows
  L = chunk_layout(pt::layout_of(chunk), b.n, 2, PartPt::kSize, 2);
  return scratch_ok(L, pt::layout_of, b.n, chunk, scratch, scratch_bytes);
}

void gi_passes(hipStream_t s, const gi_train::PassArgs &b, long long chunk, const ChunkLayout &L, float *sc, double *acc) {
  namespace gi = gi_train;
  gi::PassArgs p = b;
  p.frag = (const float4 *)(sc + L.rows.frag);
  p.rows = rows_of(sc, L.rows);
  gi::launch_prep(s, b.w.W2, (float4 *)(sc + L.rows.frag), b.valid, b.n, (int *)sc);
  for (long long c0 = 0; c0 < b.n; c0 += chunk) {
    p.n = b.n - c0 < chunk ? b.n - c0 : chunk;
    const Layout P = gi::layout_of(p.n);  // the pass's tiles and slices
    p.obs = b.obs + c0 * b.obs_stride; p.actions = b.actions + c0 * b.act_stride; p.returns = b.returns + c0 * b.ret_stride;
    p.old_logp = b.old_logp + c0; p.valid = shifted(b.valid, c0);
    p.lossp = (double *)(sc + L.lossp) + 2 * (c0 / 32);
    p.logp_out = shifted(b.logp_out, c0); p.value_out = shifted(b.value_out, c0); p.ratio_out = shifted(b.ratio_out, c0);
    gi::launch_sample(s, p);
    gi::launch_wgrad(s, p.rows, P.n_pad, P.slice_rows, P.slices, sc + L.part);
    accumulate(s, sc + L.part, P.slices, PartGi::kSize, acc);
  }
}

void pt_passes(hipStream_t s, const pt::PassArgs &b, const PtNet (&net)[2], long long chunk, const ChunkLayout &L, float *sc,
               double *acc) {
  pt::PassArgs p = b;
  p.rows = rows_of(sc, L.rows);
  pt::launch_prep(s, net[0].w ? net[0].w->W2 : nullptr, net[1].w ? net[1].w->W2 : nullptr, kHidden + b.n_a,
                  (float4 *)(sc + L.rows.frag), b.valid, b.n, (int *)sc);
  for (long long c0 = 0; c0 < b.n; c0 += chunk) {
    p.n = b.n - c0 < chunk ? b.n - c0 : chunk;
    const Layout P = pt::layout_of(p.n);  // the pass's tiles and slices
    p.obs = b.obs + c0 * b.obs_stride; p.actions = b.actions + c0 * b.act_stride; p.returns = shifted(b.returns, c0 * b.ret_stride);
    p.old_logp = shifted(b.old_logp, c0); p.valid = shifted(b.valid, c0); p.advantages = shifted(b.advantages, c0);
    for (int k = 0; k < 2; k++) {  // the actor, then the critic
      if (!net[k].w) continue;
      p.w = *net[k].w;
      p.frag = (const float4 *)(sc + L.rows.frag + k * pt::critic_frag_offset());
      p.lossp = (double *)(sc + L.lossp) + k * L.ntiles + c0 / 32;
      p.out0 = shifted(net[k].out0, c0); p.out1 = shifted(net[k].out1, c0);
      pt::launch_sample(s, k != 0, p);
      pt::launch_wgrad(s, k != 0, p.rows, P.n_pad, P.slice_rows, P.slices, sc + L.part);
      accumulate(s, sc + L.part, P.slices, PartPt::kSize, acc + k * PartPt::kSize);
    }
  }
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
  if (!weights || !complete(grads) || !loss) return MM_ERR_INVALID_ARG;
  float *sc = (float *)scratch;
  int *count = (int *)sc;  // prep's count is the one kernel A scales by
  mm::gi_train::PassArgs p = {};  // the whole batch
  p.obs = obs; p.obs_stride = obs_stride; p.n = n; p.actions = actions; p.act_stride = act_stride; p.returns = returns;
  p.ret_stride = ret_stride; p.old_logp = old_logp; p.valid = valid; p.w = *weights; p.n_a = n_a; p.clip_param = clip_param;
  p.huber = critic_loss == MM_GI_CRITIC_HUBER; p.adv_sums = adv_sums; p.count = count;
  p.logp_out = logp_taken; p.value_out = value; p.ratio_out = ratio;
  ChunkLayout L;
  if (!gi_args_ok(p, n_s, hidden, critic_loss, chunk, scratch, scratch_bytes, L)) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (!mm::gi_train::zero_grads(s, *grads, n_a) || hipMemsetAsync(loss, 0, 3 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
    return MM_OK;
  }
  double *acc = (double *)(sc + L.acc);
  if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess) return MM_ERR_DEVICE;
  if (hipMemsetAsync(acc, 0, PartGi::kSize * sizeof(double), s) != hipSuccess) return MM_ERR_DEVICE;
  gi_passes(s, p, chunk, L, sc, acc);
  const int nelem = gi_elems(n_a);
  hipLaunchKernelGGL(policy_gi_train_chunked_finish_kernel, dim3((nelem + 255) / 256 + 1), dim3(256), 0, s, (const double *)acc,
                     (int)n_a, *grads, (const double *)(sc + L.lossp), L.ntiles, (const int *)count, (int)(adv_sums != nullptr), loss);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

extern "C" int32_t mm_policy_train_chunked_scratch_bytes(int64_t n, int64_t chunk, uint64_t *bytes) {
  using namespace mm::chunked;
  if (n < 0 || n > 0x7FFFFFFF || !chunk_ok(chunk) || !bytes) return MM_ERR_INVALID_ARG;
  *bytes = (uint64_t)chunk_layout(mm::pt::layout_of(chunk), n, 2, PartPt::kSize, 2).total * 4u;
  return MM_OK;
}

extern "C" int32_t mm_policy_train_chunked(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                           int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                           const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden,
                                           int32_t n_a, float clip_param, int32_t critic_loss, const float *adv_sums,
                                           const float *advantages, const MMMlpParams *actor_grads, const MMMlpParams *critic_grads,
                                           float *loss, float *logp_taken, float *value, float *ratio, void *scratch,
                                           uint64_t scratch_bytes, MMStream stream, int64_t chunk) {
  using namespace mm::chunked;
  // everything that can refuse the call comes before the first enqueue
  if (!loss || (actor != nullptr) != (actor_grads != nullptr) || (critic != nullptr) != (critic_grads != nullptr)) return MM_ERR_INVALID_ARG;
  if ((actor_grads && !complete(actor_grads)) || (critic_grads && !complete(critic_grads))) return MM_ERR_INVALID_ARG;
  float *sc = (float *)scratch;
  int *count = (int *)sc;  // prep's count is the one kernel A scales by
  mm::pt::PassArgs p = {};  // the whole batch
  p.obs = obs; p.obs_stride = obs_stride; p.n = n; p.n_s = n_s; p.actions = actions; p.act_stride = act_stride; p.returns = returns;
  p.ret_stride = ret_stride; p.old_logp = old_logp; p.valid = valid; p.n_a = n_a; p.clip_param = clip_param;
  p.huber = critic_loss == MM_PT_CRITIC_HUBER; p.adv_sums = adv_sums; p.advantages = advantages; p.count = count;
  const PtNet net[2] = {{actor, logp_taken, ratio}, {critic, value, nullptr}};
  ChunkLayout L;
  if (!pt_args_ok(p, net, hidden, critic_loss, chunk, scratch, scratch_bytes, L)) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int k2c = kHidden + n_a;
  if (hipMemsetAsync(loss, 0, 2 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
  if (n == 0) {
    if (actor && !zero_mlp_grads(s, actor_grads, kHidden, n_s, kHidden, n_a)) return MM_ERR_DEVICE;
    if (critic && !zero_mlp_grads(s, critic_grads, kHidden, n_s, k2c, 1)) return MM_ERR_DEVICE;
    return MM_OK;
  }
  double *acc = (double *)(sc + L.acc), *lossp = (double *)(sc + L.lossp);  // the actor's, then the critic's
  if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess) return MM_ERR_DEVICE;
  if (hipMemsetAsync(acc, 0, 2 * PartPt::kSize * sizeof(double), s) != hipSuccess) return MM_ERR_DEVICE;
  pt_passes(s, p, net, chunk, L, sc, acc);
  if (actor)
    hipLaunchKernelGGL(policy_train_chunked_finish_kernel, dim3((pt_elems(n_s, kHidden, n_a) + 255) / 256 + 1), dim3(256), 0, s,
                       (const double *)acc, (int)n_s, kHidden, (int)n_a, *actor_grads, (const double *)lossp, L.ntiles,
                       (const int *)count, adv_sums ? 2 : 1, loss);
  if (critic)
    hipLaunchKernelGGL(policy_train_chunked_finish_kernel, dim3((pt_elems(n_s, k2c, 1) + 255) / 256 + 1), dim3(256), 0, s,
                       (const double *)(acc + PartPt::kSize), (int)n_s, k2c, 1, *critic_grads, (const double *)(lossp + L.ntiles),
                       L.ntiles, (const int *)count, 0, loss + 1);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
