// mm_policy_wide_chunked.hip -- the hidden-512 gradient of a whole batch under a fixed scratch budget:
// mm_policy_wide_train_chunked (include/mm_policy_wide_train.h).
//
// mm_policy_chunked.hip's design at hidden 512.  The unchunked entry keeps every sample's activations between kernel A and
// kernel B (8 384 B per sample).  Here kernels A and B -- the SAME kernels, launched through the host helpers of
// mm_policy_wide_chunked.h -- run over the batch in passes of `chunk` samples through one set of per-sample rows, and what kernel
// C folds in one go is folded across the passes:
//
//   memset     the two fp64 accumulator blocks and the count
//   prep       once, over the whole batch: both networks' W2[:, :512]^T and re-pitched W2[:, :512], and B = the number of valid
//              samples of ALL n (kernel A scales by it)
//   per pass   per network (the actor's pass, then the critic's, over the same rows): kernel A on samples [c chunk, min(n,
//              (c + 1) chunk)) (the per-sample pointers offset on the host, the loss partials at the pass's first tile of the
//              network's global array), kernel B on the pass's slices, then
//              accumulate: acc[off] += the pass's partial blocks in slice order, fp64
//   finish     per network: acc -> float in torch layout (policy_wide_fold_kernel's index map); one more workgroup folds the loss
//              partials of all ceil(n / 32) tiles with the same tree and count as the unchunked fold.
//
// A gradient element is float(the fp64 running sum of all partial blocks of all passes, in pass and slice order): exactly what
// the unchunked fold computes over its one pass, so chunk >= n gives the unchunked entry's bits.  Losses and diagnostics are per
// tile / per sample and do not depend on the slicing at all.  No floating-point atomics; only enqueues on the stream.
//
// The argument check and the pass loop are host functions (wide_args_ok, wide_passes: mm_policy_wide_chunked.h) that the
// rank-sharded entries (mm_policy_wide_sharded.hip) run too, with the caller's shard block as the accumulator.
//
// chunk is a positive multiple of 64: every pass but the last is whole 32-sample tiles (the loss partials and the diagnostics
// of a pass start on a tile boundary of the global arrays) and a slice of kernel B keeps its minimum of 2 tiles.
#include "mm_policy_wide_chunked.h"

namespace mm {
namespace wide_chunked {

using namespace mfma;
using wt::kCat;
using wt::kWide;
typedef wt::Part Part;  // one slice's partial block: 304 144 floats
static_assert(Part::kSize * 4 == MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES && Part::kSize % 2 == 0, "the header states the partial block");

// ---- accumulate: one thread per partial-block element; consecutive threads read consecutive floats of a block.
// It walks the whole block, the elements no kernel B writes included (the actor's one-hot tile of dW2: columns 512..543 of its
// 544-float rows): what lands in their accumulator slots is whatever the scratch held, and finish never reads those slots.
__global__ __launch_bounds__(256) void policy_wide_chunked_accumulate_kernel(const float *__restrict__ part, int slices,
                                                                             double *__restrict__ acc) {
  const int off = blockIdx.x * 256 + threadIdx.x;
  if (off >= Part::kSize) return;
  double s = acc[off];
#pragma unroll 8
  for (int g = 0; g < slices; g++) s += (double)part[(long long)g * Part::kSize + off];
  acc[off] = s;
}

// ---- finish: policy_wide_fold_kernel's index map (mm_policy_wide_train.hip) on the accumulator
// loss_mode 0: sum / B (critic); 1: -sum / B (actor, per-sample form); 2: -sum / B^2 (actor, reference form)
static int finish_elems(int n_s, int k2, int n_out) { return kWide * n_s + kWide + kWide * k2 + kWide + n_out * kWide + n_out; }

__global__ __launch_bounds__(256) void policy_wide_chunked_finish_kernel(const double *__restrict__ acc, int n_s, int k2, int n_out,
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
  int t = blockIdx.x * 256 + threadIdx.x;
  if (t < kWide * n_s) { const int o = t / n_s, k = t % n_s; gr.W1[t] = (float)acc[Part::kW1 + o * 32 + k]; return; }
  t -= kWide * n_s;
  if (t < kWide) { gr.b1[t] = (float)acc[Part::kb1 + t]; return; }
  t -= kWide;
  if (t < kWide * k2) { const int o = t / k2, k = t % k2; gr.W2[t] = (float)acc[Part::kW2 + o * kCat + k]; return; }
  t -= kWide * k2;
  if (t < kWide) { gr.b2[t] = (float)acc[Part::kb2 + t]; return; }
  t -= kWide;
  if (t < n_out * kWide) { gr.W3[t] = (float)acc[Part::kHd + t]; return; }
  t -= n_out * kWide;
  if (t < n_out) gr.b3[t] = (float)acc[Part::kbh + t];
}

// ---- host side (the scratch layout: mm_policy_wide_chunked.h): the argument check and the pass loop, which the entry below runs
// on the whole batch and the rank-sharded ones (mm_policy_wide_sharded.hip) on a rank's samples
static ChunkLayout chunk_layout(long long n, long long chunk) {
  ChunkLayout L;
  L.rows = wt::layout_of(chunk);
  L.ntiles = (n + 31) / 32;
  L.blocks = (int)MM_POLICY_WIDE_TRAIN_CHUNKED_BLOCKS(chunk);
  L.lossp = L.rows.lossp;  // (where the unchunked layout's own loss partials start: the end of the rows)
  L.part = L.lossp + 2 * 2 * L.ntiles;  // double[2][ntiles]
  L.acc = L.part + (long long)L.blocks * Part::kSize;
  L.total = L.acc + 2ll * 2 * Part::kSize;  // double[2][Part::kSize]
  return L;  // (total * 4 == MM_POLICY_WIDE_TRAIN_CHUNKED_BYTES(n, chunk): tests/test_wide_chunked_host.py restates the sum)
}

bool wide_args_ok(const wt::PassArgs &b, const WideNet (&net)[2], int32_t hidden, int32_t critic_loss, int64_t chunk,
                  const void *scratch, uint64_t scratch_bytes, ChunkLayout &L) {
  L = {};
  const bool actor = net[0].w != nullptr, critic = net[1].w != nullptr;
  if ((!actor && !critic) || (actor && !complete(net[0].w)) || (critic && !complete(net[1].w))) return false;
  if (!shape_ok(b.n, b.n_s, hidden, b.n_a, kWide)) return false;
  if (critic_loss != MM_PT_CRITIC_MSE && critic_loss != MM_PT_CRITIC_HUBER) return false;
  if (!(b.clip_param >= 0.0f) || !chunk_ok(chunk)) return false;
  if ((!actor && (net[0].out0 || net[0].out1)) || (!critic && net[1].out0)) return false;
  if (b.n == 0) return true;  // (empty inputs, adv_sums, advantages and the scratch are not looked at and may be NULL)
  if (!b.obs || !b.actions || b.obs_stride < b.n_s || (actor && !b.old_logp) || (critic && !b.returns)) return false;
  if (actor && ((b.adv_sums != nullptr) == (b.advantages != nullptr))) return false;
  L = chunk_layout(b.n, chunk);
  if (!scratch || ((uintptr_t)scratch & (MM_POLICY_WIDE_TRAIN_SCRATCH_ALIGN - 1)) || scratch_bytes < (uint64_t)L.total * 4u) return false;
  // the two pass sizes there are, the full one and the last one's, fit the rows and the partial blocks the size query promised
  const long long full = b.n < chunk ? b.n : (long long)chunk, last = b.n % chunk ? b.n % chunk : (long long)chunk;
  const wt::WideLayout F = wt::layout_of(full), E = wt::layout_of(last);
  return F.n_pad <= L.rows.n_pad && E.n_pad <= L.rows.n_pad && F.slices <= L.blocks && E.slices <= L.blocks;
}

void wide_passes(hipStream_t s, const wt::PassArgs &b, const WideNet (&net)[2], long long chunk, const ChunkLayout &L, float *sc,
                 double *acc) {
  wt::PassArgs p = b;
  const wt::WideRows rows = {sc + L.rows.xs, sc + L.rows.h1, sc + L.rows.h2, sc + L.rows.dz2, sc + L.rows.dz1, sc + L.rows.dh};
  p.rows = rows;
  float *part = sc + L.part;
  wt::launch_prep(s, net[0].w ? net[0].w->W2 : nullptr, net[1].w ? net[1].w->W2 : nullptr, kWide + b.n_a, sc + L.rows.w2t,
                  sc + L.rows.w2p, b.valid, b.n, (int *)sc);
  for (long long c0 = 0; c0 < b.n; c0 += chunk) {
    p.n = b.n - c0 < chunk ? b.n - c0 : chunk;
    const wt::WideLayout P = wt::layout_of(p.n);  // the pass's tiles and slices
    p.obs = b.obs + c0 * b.obs_stride; p.actions = b.actions + c0 * b.act_stride; p.returns = shifted(b.returns, c0 * b.ret_stride);
    p.old_logp = shifted(b.old_logp, c0); p.valid = shifted(b.valid, c0); p.advantages = shifted(b.advantages, c0);
    for (int k = 0; k < 2; k++) {  // the actor, then the critic
      if (!net[k].w) continue;
      p.w = *net[k].w; p.w2t = sc + L.rows.w2t + k * wt::kSquare; p.w2p = sc + L.rows.w2p + k * wt::kSquare;
      p.lossp = (double *)(sc + L.lossp) + k * L.ntiles + c0 / 32;
      p.out0 = shifted(net[k].out0, c0); p.out1 = shifted(net[k].out1, c0);
      wt::launch_sample(s, k != 0, p);
      wt::launch_wgrad(s, k != 0, rows, P.n_pad, P.slice_rows, P.slices, part);
      hipLaunchKernelGGL(policy_wide_chunked_accumulate_kernel, dim3((Part::kSize + 255) / 256), dim3(256), 0, s, (const float *)part,
                         P.slices, acc + k * Part::kSize);
    }
  }
}

}  // namespace wide_chunked
}  // namespace mm

extern "C" int32_t mm_policy_wide_train_chunked_scratch_bytes(int64_t n, int64_t chunk, uint64_t *bytes) {
  using namespace mm::wide_chunked;
  if (n < 0 || n > 0x7FFFFFFF || !chunk_ok(chunk) || !bytes) return MM_ERR_INVALID_ARG;
  *bytes = (uint64_t)chunk_layout(n, chunk).total * 4u;
  return MM_OK;
}

extern "C" int32_t mm_policy_wide_train_chunked(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                                int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                                const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic,
                                                int32_t hidden, int32_t n_a, float clip_param, int32_t critic_loss,
                                                const float *adv_sums, const float *advantages, const MMMlpParams *actor_grads,
                                                const MMMlpParams *critic_grads, float *loss, float *logp_taken, float *value,
                                                float *ratio, void *scratch, uint64_t scratch_bytes, MMStream stream, int64_t chunk) {
  using namespace mm::wide_chunked;
  namespace wt = mm::wt;
  // everything that can refuse the call comes before the first enqueue
  if (!loss || (actor != nullptr) != (actor_grads != nullptr) || (critic != nullptr) != (critic_grads != nullptr)) return MM_ERR_INVALID_ARG;
  if ((actor_grads && !complete(actor_grads)) || (critic_grads && !complete(critic_grads))) return MM_ERR_INVALID_ARG;
  float *sc = (float *)scratch;
  int *count = (int *)sc;  // prep's count is the one kernel A scales by
  wt::PassArgs p = {};  // the whole batch
  p.obs = obs; p.obs_stride = obs_stride; p.n = n; p.n_s = n_s; p.actions = actions; p.act_stride = act_stride; p.returns = returns;
  p.ret_stride = ret_stride; p.old_logp = old_logp; p.valid = valid; p.n_a = n_a; p.clip_param = clip_param;
  p.huber = critic_loss == MM_PT_CRITIC_HUBER; p.adv_sums = adv_sums; p.advantages = advantages; p.count = count;
  const WideNet net[2] = {{actor, logp_taken, ratio}, {critic, value, nullptr}};
  ChunkLayout L;
  if (!wide_args_ok(p, net, hidden, critic_loss, chunk, scratch, scratch_bytes, L)) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int k2c = kWide + n_a;
  if (hipMemsetAsync(loss, 0, 2 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
  if (n == 0) {
    if (actor && !zero_mlp_grads(s, actor_grads, kWide, n_s, kWide, n_a)) return MM_ERR_DEVICE;
    if (critic && !zero_mlp_grads(s, critic_grads, kWide, n_s, k2c, 1)) return MM_ERR_DEVICE;
    return MM_OK;
  }
  double *acc_a = (double *)(sc + L.acc), *acc_c = acc_a + Part::kSize;
  // the two networks' loss partials live side by side: both are folded at the end, after the passes alternated over the rows
  double *lossp_a = (double *)(sc + L.lossp), *lossp_c = lossp_a + L.ntiles;
  if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess) return MM_ERR_DEVICE;
  if (hipMemsetAsync(acc_a, 0, 2 * (size_t)Part::kSize * sizeof(double), s) != hipSuccess) return MM_ERR_DEVICE;
  wide_passes(s, p, net, chunk, L, sc, acc_a);
  if (actor)
    hipLaunchKernelGGL(policy_wide_chunked_finish_kernel, dim3((finish_elems(n_s, kWide, n_a) + 255) / 256 + 1), dim3(256), 0, s,
                       (const double *)acc_a, (int)n_s, kWide, (int)n_a, *actor_grads, (const double *)lossp_a, L.ntiles,
                       (const int *)count, adv_sums ? 2 : 1, loss);
  if (critic)
    hipLaunchKernelGGL(policy_wide_chunked_finish_kernel, dim3((finish_elems(n_s, k2c, 1) + 255) / 256 + 1), dim3(256), 0, s,
                       (const double *)acc_c, (int)n_s, k2c, 1, *critic_grads, (const double *)lossp_c, L.ntiles, (const int *)count, 0,
                       loss + 1);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
