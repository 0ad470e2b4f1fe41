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

// ---- host side
// The chunked scratch, offsets in floats: the header, the four [512][512] blocks and the per-sample rows as in the unchunked
// layout of `chunk` samples; then the fp64 loss partials of all ceil(n / 32) tiles of the actor and of the critic, the partial
// blocks of one pass, and the two fp64 accumulator blocks.
// The partial blocks hold the most slices ANY pass of at most `chunk` samples cuts, not the slices of a full pass: under the
// header's rule a pass of t tiles cuts ceil(t / max(2, ceil(t / 48))) slices, never more than 48 nor than ceil(t / 2), and a
// shorter last pass can cut more than a full one (98 tiles: 33 slices of 3; 96 tiles: 48 slices of 2).
struct ChunkLayout {
  wt::WideLayout rows;  // the unchunked layout of `chunk` samples: w2t, w2p, xs .. dh
  long long ntiles, lossp, part, acc, total;
  int blocks;
};

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
  if ((!actor && !critic) || !loss) return MM_ERR_INVALID_ARG;
  if ((actor != nullptr) != (actor_grads != nullptr) || (critic != nullptr) != (critic_grads != nullptr)) return MM_ERR_INVALID_ARG;
  if ((actor && (!complete(actor) || !complete(actor_grads))) || (critic && (!complete(critic) || !complete(critic_grads))))
    return MM_ERR_INVALID_ARG;
  if (!shape_ok(n, n_s, hidden, n_a, kWide)) return MM_ERR_INVALID_ARG;
  if (critic_loss != MM_PT_CRITIC_MSE && critic_loss != MM_PT_CRITIC_HUBER) return MM_ERR_INVALID_ARG;
  if (!(clip_param >= 0.0f) || !chunk_ok(chunk)) return MM_ERR_INVALID_ARG;
  if ((!actor && (logp_taken || ratio)) || (!critic && value)) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int k2c = kWide + n_a;
  // everything that can refuse the call comes before the first enqueue
  ChunkLayout L = {};
  if (n > 0) {
    if (!obs || !actions || obs_stride < n_s || (actor && !old_logp) || (critic && !returns)) return MM_ERR_INVALID_ARG;
    if (actor && ((adv_sums != nullptr) == (advantages != nullptr))) return MM_ERR_INVALID_ARG;
    L = chunk_layout(n, chunk);
    if (!scratch || ((uintptr_t)scratch & (MM_POLICY_WIDE_TRAIN_SCRATCH_ALIGN - 1)) || scratch_bytes < (uint64_t)L.total * 4u)
      return MM_ERR_INVALID_ARG;
    // the two pass sizes there are, the full one and the last one's, fit the rows and the partial blocks the size query promised
    const long long full = n < chunk ? n : (long long)chunk, last = n % chunk ? n % chunk : (long long)chunk;
    const wt::WideLayout F = wt::layout_of(full), E = wt::layout_of(last);
    if (F.n_pad > L.rows.n_pad || E.n_pad > L.rows.n_pad || F.slices > L.blocks || E.slices > L.blocks) return MM_ERR_INVALID_ARG;
  }
  if (hipMemsetAsync(loss, 0, 2 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
  if (n == 0) {
    if (actor && !zero_mlp_grads(s, actor_grads, kWide, n_s, kWide, n_a)) return MM_ERR_DEVICE;
    if (critic && !zero_mlp_grads(s, critic_grads, kWide, n_s, k2c, 1)) return MM_ERR_DEVICE;
    return MM_OK;
  }
  float *sc = (float *)scratch;
  int *count = (int *)sc;
  double *acc_a = (double *)(sc + L.acc), *acc_c = acc_a + Part::kSize;
  // the two networks' loss partials live side by side: both are folded at the end, after the passes alternated over the rows
  double *lossp_a = (double *)(sc + L.lossp), *lossp_c = lossp_a + L.ntiles;
  if (hipMemsetAsync(count, 0, sizeof(int), s) != hipSuccess) return MM_ERR_DEVICE;
  if (hipMemsetAsync(acc_a, 0, 2 * (size_t)Part::kSize * sizeof(double), s) != hipSuccess) return MM_ERR_DEVICE;
  wt::launch_prep(s, actor ? actor->W2 : nullptr, critic ? critic->W2 : nullptr, k2c, sc + L.rows.w2t, sc + L.rows.w2p, valid,
                  (long long)n, count);
  wt::PassArgs p = {};
  p.obs_stride = obs_stride; p.n_s = n_s; p.act_stride = act_stride; p.ret_stride = ret_stride; p.n_a = n_a;
  p.clip_param = clip_param; p.huber = critic_loss == MM_PT_CRITIC_HUBER; p.adv_sums = adv_sums; p.count = count;
  const wt::WideRows rows = {sc + L.rows.xs, sc + L.rows.h1, sc + L.rows.h2, sc + L.rows.dz2, sc + L.rows.dz1, sc + L.rows.dh};
  p.rows = rows;
  float *part = sc + L.part;
  for (long long c0 = 0; c0 < n; c0 += chunk) {
    const long long np = n - c0 < chunk ? n - c0 : (long long)chunk;
    const wt::WideLayout P = wt::layout_of(np);  // the pass's tiles and slices
    p.n = np;
    p.obs = obs + c0 * obs_stride; p.actions = actions + c0 * act_stride; p.returns = shifted(returns, c0 * ret_stride);
    p.old_logp = shifted(old_logp, c0); p.valid = shifted(valid, c0); p.advantages = shifted(advantages, c0);
    if (actor) {
      p.w = *actor; p.w2t = sc + L.rows.w2t; p.w2p = sc + L.rows.w2p; p.lossp = lossp_a + c0 / 32;
      p.out0 = shifted(logp_taken, c0); p.out1 = shifted(ratio, c0);
      wt::launch_sample(s, false, p);
      wt::launch_wgrad(s, false, rows, P.n_pad, P.slice_rows, P.slices, part);
      hipLaunchKernelGGL(policy_wide_chunked_accumulate_kernel, dim3((Part::kSize + 255) / 256), dim3(256), 0, s, (const float *)part,
                         P.slices, acc_a);
    }
    if (critic) {
      p.w = *critic; p.w2t = sc + L.rows.w2t + wt::kSquare; p.w2p = sc + L.rows.w2p + wt::kSquare; p.lossp = lossp_c + c0 / 32;
      p.out0 = shifted(value, c0); p.out1 = nullptr;
      wt::launch_sample(s, true, p);
      wt::launch_wgrad(s, true, rows, P.n_pad, P.slice_rows, P.slices, part);
      hipLaunchKernelGGL(policy_wide_chunked_accumulate_kernel, dim3((Part::kSize + 255) / 256), dim3(256), 0, s, (const float *)part,
                         P.slices, acc_c);
    }
  }
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
