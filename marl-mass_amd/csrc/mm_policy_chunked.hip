// mm_policy_chunked.hip -- the gradient of a whole batch under a fixed scratch budget: mm_policy_gi_train_chunked
// (include/mm_policy_gi_train.h), mm_policy_train_chunked (include/mm_policy_train.h) and, at hidden 512,
// mm_policy_wide_train_chunked (include/mm_policy_wide_train.h).
//
// The unchunked entries keep every sample's activations between kernel A and kernel B (2 496 B / 2 240 B / 8 384 B per sample).
// Here kernels A and B -- the SAME kernels, launched through the host helpers of mm_policy_chunked.h -- run over the batch in passes
// of `chunk` samples through one set of per-sample rows, and what kernel C folds in one go is folded across the passes:
//
//   memset     the fp64 accumulator block(s) and the count
//   prep       once, over the whole batch: the W2^T fragments (512: both networks' W2[:, :512]^T and re-pitched W2[:, :512]) and
//              B = the number of valid samples of ALL n (kernel A scales by it)
//   per pass   kernel A on samples [c chunk, min(n, (c + 1) chunk)) (the per-sample pointers offset on the host, the loss
//              partials at the pass's first tile of the global array), kernel B on the pass's slices, then
//              accumulate: acc[off] += the pass's partial blocks in workgroup order, fp64
//   finish     acc -> float in torch layout (the index maps of the fold kernels); one more workgroup folds the loss partials
//              of all ceil(n / 32) tiles with the same tree and count as the unchunked fold.
//
// A gradient element is float(the fp64 running sum of all partial blocks of all passes, in pass and workgroup order): exactly
// what the unchunked fold computes over its one pass, so chunk >= n gives the unchunked entry's bits.  Losses and diagnostics are
// per tile / per sample and do not depend on the slicing at all.  No floating-point atomics; only enqueues on the stream.
//
// chunk is a positive multiple of 64: every pass but the last is whole 32-sample tiles (the loss partials and the diagnostics
// of a pass start on a tile boundary of the global arrays) and a slice of kernel B keeps its minimum of 2 tiles.
//
// The separate actor and critic are written once for both hidden sizes, against the traits Pt128 and Pt512 (mm_policy_chunked.h).
#include "mm_policy_chunked.h"

namespace mm {
namespace chunked {

using namespace mfma;

// ---- accumulate: one thread per partial-block element; consecutive threads read consecutive floats of a block.
// It walks the whole block, the elements no kernel B writes included (the actor's one-hot tile of dW2: columns 128..159 of its
// 160-float rows, 512..543 of 544 at hidden 512): what lands in their accumulator slots is whatever the scratch held, and finish
// never reads those slots.
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

// ---- finish, one separate network: grad_slot<F>'s index map (mm_policy_chunked.h) on the accumulator
// loss_mode 0: sum / B (critic); 1: -sum / B (actor, per-sample form); 2: -sum / B^2 (actor, reference form)
template <class F>
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
  float *dst = grad_slot<F>(blockIdx.x * 256 + threadIdx.x, n_s, k2, n_out, gr, src);
  if (dst) *dst = (float)acc[src];
}

// ---- host side (the scratch layout: mm_policy_chunked.h): the accumulate launch, then each family's argument check and pass
// loop, which the entries below run on the whole batch and the rank-sharded ones (mm_policy_sharded.hip) on a rank's samples
void accumulate(hipStream_t s, const float *part, int slices, int size, double *acc) {
  hipLaunchKernelGGL(train_chunked_accumulate_kernel, dim3((size + 255) / 256), dim3(256), 0, s, part, slices, size, acc);
}

template <class Rows>
static bool scratch_ok(const ChunkLayout<Rows> &L, Rows (*layout_of)(long long), uintptr_t align, long long n, long long chunk,
                       const void *scratch, uint64_t scratch_bytes) {
  if (!scratch || ((uintptr_t)scratch & (align - 1)) || scratch_bytes < (uint64_t)L.total * 4u) return false;
  // the two pass sizes there are, the full one and the last one's, fit the rows and the partial blocks the size query promised
  const Rows F = layout_of(n < chunk ? n : chunk), E = layout_of(n % chunk ? n % chunk : chunk);
  return F.n_pad <= L.rows.n_pad && E.n_pad <= L.rows.n_pad && F.slices <= L.blocks && E.slices <= L.blocks;
}

static ChunkLayout<Layout> gi_chunk_layout(long long n, long long chunk) {
  const Layout rows = gi_train::layout_of(chunk);
  return chunk_layout(rows, n, narrow_blocks(rows), PartGi::kSize, 1);
}

bool gi_args_ok(const gi_train::PassArgs &b, int32_t n_s, int32_t hidden, int32_t critic_loss, int64_t chunk, const void *scratch,
                uint64_t scratch_bytes, ChunkLayout<Layout> &L) {
  L = {};
  if (!complete(&b.w) || !shape_ok(b.n, n_s, hidden, b.n_a, kHidden)) return false;
  if (critic_loss != MM_GI_CRITIC_MSE && critic_loss != MM_GI_CRITIC_HUBER) return false;
  if (!(b.clip_param >= 0.0f) || !chunk_ok(chunk)) return false;
  if (b.n == 0) return true;  // (empty inputs and the scratch are not looked at and may be NULL)
  if (!b.obs || !b.actions || !b.returns || !b.old_logp || b.obs_stride < n_s) return false;
  L = gi_chunk_layout(b.n, chunk);
  return scratch_ok(L, gi_train::layout_of, 16, b.n, chunk, scratch, scratch_bytes);
}

template <class F>
bool args_ok(const typename F::PassArgs &b, const Net (&net)[2], int32_t hidden, int32_t critic_loss, int64_t chunk, const void *scratch,
             uint64_t scratch_bytes, ChunkLayout<typename F::Layout> &L) {
  L = {};
  const bool actor = net[0].w != nullptr, critic = net[1].w != nullptr;
  if ((!actor && !critic) || (actor && !complete(net[0].w)) || (critic && !complete(net[1].w))) return false;
  if (!shape_ok(b.n, b.n_s, hidden, b.n_a, F::kHid)) return false;
  if (critic_loss != MM_PT_CRITIC_MSE && critic_loss != MM_PT_CRITIC_HUBER) return false;
  if (!(b.clip_param >= 0.0f) || !chunk_ok(chunk)) return false;
  if ((!actor && (net[0].out0 || net[0].out1)) || (!critic && net[1].out0)) return false;
  if (b.n == 0) return true;  // (empty inputs, adv_sums, advantages and the scratch are not looked at and may be NULL)
  if (!b.obs || !b.actions || b.obs_stride < b.n_s || (actor && !b.old_logp) || (critic && !b.returns)) return false;
  if (actor && ((b.adv_sums != nullptr) == (b.advantages != nullptr))) return false;
  // the two networks' loss partials live side by side: both are folded at the end, after the passes alternated over the rows
  L = chunk_layout_of<F>(b.n, chunk);
  return scratch_ok(L, F::layout_of, F::kAlign, b.n, chunk, scratch, scratch_bytes);
}

void gi_passes(hipStream_t s, const gi_train::PassArgs &b, long long chunk, const ChunkLayout<Layout> &L, float *sc, double *acc) {
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

template <class F>
void passes(hipStream_t s, const typename F::PassArgs &b, const Net (&net)[2], long long chunk, const ChunkLayout<typename F::Layout> &L,
            float *sc, double *acc) {
  typedef typename F::Part Part;
  typename F::PassArgs p = b;
  F::prep(s, net[0].w ? net[0].w->W2 : nullptr, net[1].w ? net[1].w->W2 : nullptr, F::kHid + b.n_a, sc, L.rows, b.valid, b.n);
  for (long long c0 = 0; c0 < b.n; c0 += chunk) {
    p.n = b.n - c0 < chunk ? b.n - c0 : chunk;
    const typename F::Layout P = F::layout_of(p.n);  // the pass's tiles and slices
    p.obs = b.obs + c0 * b.obs_stride; p.actions = b.actions + c0 * b.act_stride; p.returns = shifted(b.returns, c0 * b.ret_stride);
    p.old_logp = shifted(b.old_logp, c0); p.valid = shifted(b.valid, c0); p.advantages = shifted(b.advantages, c0);
    for (int k = 0; k < 2; k++) {  // the actor, then the critic
      if (!net[k].w) continue;
      p.w = *net[k].w;
      F::bind(p, sc, L.rows, k);
      p.lossp = (double *)(sc + L.lossp) + k * L.ntiles + c0 / 32;
      p.out0 = shifted(net[k].out0, c0); p.out1 = shifted(net[k].out1, c0);
      F::sample(s, k != 0, p);
      F::wgrad(s, k != 0, p, P, sc + L.part);
      accumulate(s, sc + L.part, P.slices, Part::kSize, acc + k * Part::kSize);
    }
  }
}

template bool args_ok<Pt128>(const pt::PassArgs &, const Net (&)[2], int32_t, int32_t, int64_t, const void *, uint64_t, ChunkLayout<Layout> &);
template bool args_ok<Pt512>(const wt::PassArgs &, const Net (&)[2], int32_t, int32_t, int64_t, const void *, uint64_t,
                             ChunkLayout<wt::WideLayout> &);
template void passes<Pt128>(hipStream_t, const pt::PassArgs &, const Net (&)[2], long long, const ChunkLayout<Layout> &, float *, double *);
template void passes<Pt512>(hipStream_t, const wt::PassArgs &, const Net (&)[2], long long, const ChunkLayout<wt::WideLayout> &, float *,
                            double *);

// ---- the separate networks' chunked entry and its size query at hidden F::kHid
template <class F>
static int32_t train_chunked_scratch_bytes(int64_t n, int64_t chunk, uint64_t *bytes) {
  if (n < 0 || n > 0x7FFFFFFF || !chunk_ok(chunk) || !bytes) return MM_ERR_INVALID_ARG;
  *bytes = (uint64_t)chunk_layout_of<F>(n, chunk).total * 4u;
  return MM_OK;
}

template <class F>
static int32_t train_chunked(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions, int64_t act_stride,
                             const float *returns, int64_t ret_stride, const float *old_logp, const uint8_t *valid,
                             const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden, int32_t n_a, float clip_param,
                             int32_t critic_loss, const float *adv_sums, const float *advantages, const MMMlpParams *actor_grads,
                             const MMMlpParams *critic_grads, float *loss, float *logp_taken, float *value, float *ratio, void *scratch,
                             uint64_t scratch_bytes, MMStream stream, int64_t chunk) {
  typedef typename F::Part Part;
  // everything that can refuse the call comes before the first enqueue
  if (!loss || (actor != nullptr) != (actor_grads != nullptr) || (critic != nullptr) != (critic_grads != nullptr)) return MM_ERR_INVALID_ARG;
  if ((actor_grads && !complete(actor_grads)) || (critic_grads && !complete(critic_grads))) return MM_ERR_INVALID_ARG;
  float *sc = (float *)scratch;
  int *count = (int *)sc;  // prep's count is the one kernel A scales by
  typename F::PassArgs p = {};  // the whole batch
  p.obs = obs; p.obs_stride = obs_stride; p.n = n; p.n_s = n_s; p.actions = actions; p.act_stride = act_stride; p.returns = returns;
  p.ret_stride = ret_stride; p.old_logp = old_logp; p.valid = valid; p.n_a = n_a; p.clip_param = clip_param;
  p.huber = critic_loss == MM_PT_CRITIC_HUBER; p.adv_sums = adv_sums; p.advantages = advantages; p.count = count;
  const Net net[2] = {{actor, logp_taken, ratio}, {critic, value, nullptr}};
  const MMMlpParams *const grads[2] = {actor_grads, critic_grads};
  ChunkLayout<typename F::Layout> L;
  if (!args_ok<F>(p, net, hidden, critic_loss, chunk, scratch, scratch_bytes, L)) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int k2[2] = {F::kHid, F::kHid + n_a}, n_out[2] = {n_a, 1};  // the actor's and the critic's fc2 row and outputs
  if (hipMemsetAsync(loss, 0, 2 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
  if (n == 0) {
    for (int k = 0; k < 2; k++)
      if (grads[k] && !zero_mlp_grads(s, grads[k], F::kHid, n_s, k2[k], n_out[k])) return MM_ERR_DEVICE;
    return MM_OK;
  }
  double *acc = (double *)(sc + L.acc), *lossp = (double *)(sc + L.lossp);  // the actor's, then the critic's
  if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess) return MM_ERR_DEVICE;
  if (hipMemsetAsync(acc, 0, 2 * (size_t)Part::kSize * sizeof(double), s) != hipSuccess) return MM_ERR_DEVICE;
  passes<F>(s, p, net, chunk, L, sc, acc);
  for (int k = 0; k < 2; k++) {
    if (!grads[k]) continue;
    hipLaunchKernelGGL(policy_train_chunked_finish_kernel<F>, dim3((grad_elems<F>(n_s, k2[k], n_out[k]) + 255) / 256 + 1), dim3(256), 0,
                       s, (const double *)(acc + k * Part::kSize), (int)n_s, k2[k], n_out[k], *grads[k],
                       (const double *)(lossp + k * L.ntiles), L.ntiles, (const int *)count, k ? 0 : (adv_sums ? 2 : 1), loss + k);
  }
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

}  // namespace chunked
}  // namespace mm

extern "C" int32_t mm_policy_gi_train_chunked_scratch_bytes(int64_t n, int64_t chunk, uint64_t *bytes) {
  using namespace mm::chunked;
  if (n < 0 || n > 0x7FFFFFFF || !chunk_ok(chunk) || !bytes) return MM_ERR_INVALID_ARG;
  *bytes = (uint64_t)gi_chunk_layout(n, chunk).total * 4u;
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
  ChunkLayout<Layout> L;
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
  return mm::chunked::train_chunked_scratch_bytes<mm::chunked::Pt128>(n, chunk, bytes);
}

extern "C" int32_t mm_policy_wide_train_chunked_scratch_bytes(int64_t n, int64_t chunk, uint64_t *bytes) {
  return mm::chunked::train_chunked_scratch_bytes<mm::chunked::Pt512>(n, chunk, bytes);
}

extern "C" int32_t mm_policy_train_chunked(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                           int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                           const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden,
                                           int32_t n_a, float clip_param, int32_t critic_loss, const float *adv_sums,
                                           const float *advantages, const MMMlpParams *actor_grads, const MMMlpParams *critic_grads,
                                           float *loss, float *logp_taken, float *value, float *ratio, void *scratch,
                                           uint64_t scratch_bytes, MMStream stream, int64_t chunk) {
  return mm::chunked::train_chunked<mm::chunked::Pt128>(obs, obs_stride, n, n_s, actions, act_stride, returns, ret_stride, old_logp, valid,
                                                        actor, critic, hidden, n_a, clip_param, critic_loss, adv_sums, advantages,
                                                        actor_grads, critic_grads, loss, logp_taken, value, ratio, scratch, scratch_bytes,
                                                        stream, chunk);
}

extern "C" int32_t mm_policy_wide_train_chunked(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                                int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                                const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic,
                                                int32_t hidden, int32_t n_a, float clip_param, int32_t critic_loss,
                                                const float *adv_sums, const float *advantages, const MMMlpParams *actor_grads,
                                                const MMMlpParams *critic_grads, float *loss, float *logp_taken, float *value,
                                                float *ratio, void *scratch, uint64_t scratch_bytes, MMStream stream, int64_t chunk) {
  return mm::chunked::train_chunked<mm::chunked::Pt512>(obs, obs_stride, n, n_s, actions, act_stride, returns, ret_stride, old_logp, valid,
                                                        actor, critic, hidden, n_a, clip_param, critic_loss, adv_sums, advantages,
                                                        actor_grads, critic_grads, loss, logp_taken, value, ratio, scratch, scratch_bytes,
                                                        stream, chunk);
}
