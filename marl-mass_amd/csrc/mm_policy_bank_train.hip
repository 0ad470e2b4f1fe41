// mm_policy_bank_train.hip -- K actor / critic pairs of one shape, each on its own column group of one batch: the forward
// evaluation (mm_policy_bank_eval) and the loss and full gradient (mm_policy_bank_train) of include/mm_policy_bank_train.h.
//
// The arithmetic is mm_policy_train.hip's, from the pieces of mm_policy_mfma.h, and the decomposition of every group is
// mm_policy_train's on that group's n_k samples; what differs is where a tile's inputs and scratch rows live and whose weights a
// workgroup stages.  Kernel A is the text mm_policy_train.hip runs, mlp_sample_kernel of mm_policy_sample.h, with that difference as
// its policy `Group`; kernel B is wgrad_rows and kernel C fold / loss_tree, on the group's own rows, partial blocks and tiles.
//
//   frag      W2[:, :128]^T of every member's given networks in MFMA A-fragment order (128 KB per member).
//   stats     per 32-sample tile of a group, in fp64: the number of valid samples and the sums of the non-negative and of the
//             negative advantages (a fixed butterfly); stats_fold: one workgroup per group folds its tiles in loss_tree's
//             fixed tree into B_k and the float S+_k, S-_k.
//   kernel A  a workgroup belongs to ONE group (the block prefix table of mm_policy_bank_grid on the n_k): it stages that
//             member's fragments once and walks the group's tiles, counted from the group's own start.  Member-local
//             sample i = 32 tile + lane sits at row i / w_k, column col_start[k] + i % w_k of the batch; its scratch rows at
//             32 tile_start[k] + i.
//   kernel B  grid = the sum of the groups' slices; a workgroup finds its group from the slice prefix table.
//   kernel C  grid (elements, K): member k folds its own partial blocks in workgroup order, the last workgroup its loss tree.
// The tables ride in the by-value argument blocks (uniform lookups: scalar loads from the kernel-argument segment).
#include "mm_policy_sample.h"  // kernel A; mm_policy_mfma.h
#include "mm_policy_bank_tables.h"  // Tables, group_of, sample_of, the statistics, plan: shared with mm_policy_gi_bank_train.hip
#include "../../include/mm_policy_bank_train.h"

namespace mm {
namespace bank_train {

using namespace mfma;
constexpr int kWavesA = MM_BANK_WAVES;  // kernel A's 8 waves, as policy_bank_kernel's: mm_policy_bank_grid splits the workgroups
static_assert(kThreadsA == 64 * kWavesA, "kernel A's workgroup");
constexpr int kThreadsB = 320;
constexpr long long kFrag = 4 * 4 * 4 * 64 * 4;  // W2^T fragments of one network, in floats
typedef PartialBlock<4> Part;
static_assert(MM_BANK_TILE == 32, "one wave per 32 samples: the MFMA tile");
static_assert(2 * kFrag * 4 == MM_PBT_MEMBER_BYTES && Part::kSize * 4 == MM_PBT_PARTIAL_BYTES, "the header's scratch figures");
static_assert((4 * kHidden + kDh + kXs) * 4 == MM_PBT_SAMPLE_BYTES && MM_PBT_HEADER_BYTES == 4 * 4 * kG, "the header's scratch figures");

// ---- frag: W2[:, :128]^T fragments of member blockIdx.y's given networks
__global__ __launch_bounds__(256) void bank_frag_kernel(const float *__restrict__ W2a, const float *__restrict__ W2c, int k2c,
                                                        float4 *__restrict__ frag) {
  const int t = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  const bool crit = t >= 4096;
  const float *W2 = crit ? W2c : W2a;
  const int k2 = crit ? k2c : kHidden;
  if (W2) frag[(long long)k * 2 * 4096 + t] = w2t_fragment(W2 + (long long)k * kHidden * k2, k2, t & 4095);
}

// ---- stats: one wave per tile, lanes 0..31 one sample each; stats_fold: one workgroup per group (mm_policy_bank_tables.h)
__global__ __launch_bounds__(256) void bank_stats_kernel(const StatArgs p, const Tables tb, int total_tiles) {
  stats_tiles(p, tb, total_tiles);
}

__global__ __launch_bounds__(256) void bank_stats_fold_kernel(const double *__restrict__ stats, const Tables tb, int *__restrict__ count,
                                                              float *__restrict__ sums, float *__restrict__ sums_out) {
  stats_fold(stats, tb, count, sums, sums_out);
}

struct SampleArgs {
  const float *obs;
  long long obs_stride;
  int n_s;
  const int32_t *actions;
  long long act_stride;
  const float *returns;
  long long ret_stride;
  const float *old_logp;
  const uint8_t *valid;
  MMMlpParams w;  // the six stacked bases
  int n_a;
  float clip_param;
  int huber, ref_form;
  const float *adv_sums;  // [K][2]
  const float *advantages, *target_value;
  const int *count;    // [K]
  const float4 *frag;  // this network's fragments of member 0; member k 2 * 4096 float4 further
  float *s_h1, *s_dz1, *s_h2, *s_dz2, *s_dh, *s_xs;
  double *lossp;
  float *out0, *out1;  // actor: logp_taken, ratio; critic: value, unused
};

// ---- kernel A: mlp_sample_kernel of mm_policy_sample.h; a workgroup serves the group its index falls in
struct Group {
  const SampleArgs &p;
  int g, lb, nblk;           // the workgroup's group = member, its index among the group's workgroups, and their number
  unsigned c0, gw, row_len;  // the group's first column and its width
  long long n_, row_base;    // the group's samples and its first scratch row
  MM_DEV Group(const SampleArgs &a, const Tables &tb) : p(a) {
    const int b = (int)blockIdx.x;
    g = group_of(tb.block_start, b);
    lb = b - tb.block_start[g]; nblk = tb.block_start[g + 1] - tb.block_start[g];
    c0 = tb.col_start[g]; gw = tb.col_start[g + 1] - c0; row_len = tb.row_len;
    n_ = (long long)gw * tb.rows; row_base = 32ll * tb.tile_start[g];
  }
  MM_DEV MMMlpParams net(int n_s, int k2, int n_out) const {  // member g of the stacked tensors
    return {p.w.W1 + (long long)g * kHidden * n_s, p.w.b1 + g * kHidden, p.w.W2 + (long long)g * kHidden * k2, p.w.b2 + g * kHidden,
            p.w.W3 + g * n_out * kHidden, p.w.b3 + g * n_out};
  }
  MM_DEV const float4 *frag() const { return p.frag + (long long)g * 2 * 4096; }
  MM_DEV double *lossp() const { return p.lossp + (row_base >> 5); }
  MM_DEV long long n() const { return n_; }
  MM_DEV long long first_tile(int wave) const { return (long long)lb * kWavesA + wave; }  // tiles are counted from the group's start
  MM_DEV long long tile_stride() const { return (long long)nblk * kWavesA; }
  MM_DEV int count() const { return p.count[g]; }
  MM_DEV const float *adv_sums() const { return p.adv_sums + 2 * g; }
  MM_DEV bool ref_form() const { return p.ref_form != 0; }
  MM_DEV long long sample(long long i, bool in_range) const { return in_range ? (long long)sample_of((unsigned)i, gw, c0, row_len) : 0; }
  MM_DEV long long row(long long i) const { return row_base + i; }
  MM_DEV float advantage(long long ag) const { return p.advantages ? p.advantages[ag] : p.returns[ag * p.ret_stride] - p.target_value[ag]; }
};

template <bool kCritic, bool kTrain>
constexpr auto bank_sample_kernel = mlp_sample_kernel<kCritic, kTrain, Group, SampleArgs, Tables>;

// ---- kernel B: workgroup b = slice b - slice_start[g] of group g
template <bool kCritic>
__global__ __launch_bounds__(kThreadsB) void bank_wgrad_kernel(const float *__restrict__ s_h1, const float *__restrict__ s_dz1,
                                                               const float *__restrict__ s_h2, const float *__restrict__ s_dz2,
                                                               const float *__restrict__ s_dh, const float *__restrict__ s_xs,
                                                               const Tables tb, float *__restrict__ part) {
  const int b = (int)blockIdx.x;
  const int g = group_of(tb.slice_start, b);
  const int nt = tb.tile_start[g + 1] - tb.tile_start[g];
  const long long slice_rows = 32ll * tiles_per_slice(nt);
  const long long row0 = 32ll * tb.tile_start[g] + (long long)(b - tb.slice_start[g]) * slice_rows;
  long long row1 = row0 + slice_rows;
  if (row1 > 32ll * tb.tile_start[g + 1]) row1 = 32ll * tb.tile_start[g + 1];
  wgrad_rows<4, kCritic>(s_h1, s_dz1, s_h2, s_dz2, s_dh, s_xs, row0, row1, part + (long long)b * Part::kSize);
}

// ---- kernel C: member blockIdx.y; element t = its partial blocks summed in workgroup order; the last workgroup folds its loss
__global__ __launch_bounds__(256) void bank_fold_kernel(const float *__restrict__ part_all, const Tables tb, int n_s, int k2, int n_out,
                                                        MMMlpParams gr, const double *__restrict__ lossp, const int *__restrict__ count,
                                                        int loss_mode, float *__restrict__ loss) {
  const int k = blockIdx.y;
  if (blockIdx.x == gridDim.x - 1) {
    __shared__ double ssum[1][256];
    const int nt = tb.tile_start[k + 1] - tb.tile_start[k];
    loss_tree<1>(lossp + tb.tile_start[k], nt, ssum);
    if (threadIdx.x == 0) {
      const double inv = inv_count(count + k);
      const float v = (float)(loss_mode == 0 ? ssum[0][0] * inv : (loss_mode == 1 ? -ssum[0][0] * inv : -ssum[0][0] * inv * inv));
      loss[2 * k] = nt > 0 ? v : 0.0f;
    }
    return;
  }
  const float *part = part_all + (long long)tb.slice_start[k] * Part::kSize;
  const int slices = tb.slice_start[k + 1] - tb.slice_start[k];
  int t = blockIdx.x * 256 + threadIdx.x;
  if (t < kHidden * n_s) { const int o = t / n_s, c = t % n_s; gr.W1[(long long)k * kHidden * n_s + t] = fold<Part::kSize>(part, slices, Part::kW1 + o * 32 + c); return; }
  t -= kHidden * n_s;
  if (t < kHidden) { gr.b1[k * kHidden + t] = fold<Part::kSize>(part, slices, Part::kb1 + t); return; }
  t -= kHidden;
  if (t < kHidden * k2) { const int o = t / k2, c = t % k2; gr.W2[(long long)k * kHidden * k2 + t] = fold<Part::kSize>(part, slices, Part::kW2 + o * kW2Pitch + c); return; }
  t -= kHidden * k2;
  if (t < kHidden) { gr.b2[k * kHidden + t] = fold<Part::kSize>(part, slices, Part::kb2 + t); return; }
  t -= kHidden;
  if (t < n_out * kHidden) { gr.W3[k * n_out * kHidden + t] = fold<Part::kSize>(part, slices, Part::kHd + t); return; }
  t -= n_out * kHidden;
  if (t < n_out) gr.b3[k * n_out + t] = fold<Part::kSize>(part, slices, Part::kbh + t);
}

// ---- host side
// the scratch, offsets in floats
struct Scratch {
  long long count, sums, frag, h1, dz1, h2, dz2, dh, xs, lossp, stats, part, total;
};

static Scratch scratch_of(const Plan &P, int K) {
  Scratch S;
  const long long n_pad = 32 * P.total_tiles;
  S.count = 0;
  S.sums = kG;
  S.frag = MM_PBT_HEADER_BYTES / 4;
  S.h1 = S.frag + (long long)K * 2 * kFrag;
  S.dz1 = S.h1 + n_pad * kHidden;
  S.h2 = S.dz1 + n_pad * kHidden;
  S.dz2 = S.h2 + n_pad * kHidden;
  S.dh = S.dz2 + n_pad * kHidden;
  S.xs = S.dh + n_pad * kDh;
  S.lossp = S.xs + n_pad * kXs;
  S.stats = S.lossp + 2 * P.total_tiles;
  S.part = S.stats + 6 * P.total_tiles;
  S.total = S.part + P.cap_slices * Part::kSize;
  return S;
}

}  // namespace bank_train
}  // namespace mm

extern "C" int32_t mm_policy_bank_eval(const float *obs, int64_t obs_stride, int64_t rows, int64_t row_len, int32_t n_s,
                                       const int32_t *actions, int64_t act_stride, const uint8_t *valid, const MMMlpParams *actors,
                                       const MMMlpParams *critics, int32_t K, const int64_t *col_start, int32_t hidden, int32_t n_a,
                                       float *logp_taken, float *value, MMStream stream) {
  using namespace mm::bank_train;
  if (!actors && !critics) return MM_ERR_INVALID_ARG;
  if ((actors && !complete(actors)) || (critics && !complete(critics))) return MM_ERR_INVALID_ARG;
  Plan P;
  if (!plan(rows, row_len, K, col_start, true, P) || !shape_ok(P.n, n_s, hidden, n_a, kHidden)) return MM_ERR_INVALID_ARG;
  if (P.n == 0) return MM_OK;
  if ((actors != nullptr) != (logp_taken != nullptr) || (critics != nullptr) != (value != nullptr)) return MM_ERR_INVALID_ARG;
  if (!obs || !actions || obs_stride < n_s) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  SampleArgs a = {};
  a.obs = obs; a.obs_stride = obs_stride; a.n_s = n_s; a.actions = actions; a.act_stride = act_stride; a.valid = valid; a.n_a = n_a;
  const unsigned grid = (unsigned)P.tb.block_start[K];
  if (actors) {
    a.w = *actors; a.out0 = logp_taken;
    hipLaunchKernelGGL((bank_sample_kernel<false, false>), dim3(grid), dim3(kThreadsA), 0, s, a, P.tb);
  }
  if (critics) {
    a.w = *critics; a.out0 = value;
    hipLaunchKernelGGL((bank_sample_kernel<true, false>), dim3(grid), dim3(kThreadsA), 0, s, a, P.tb);
  }
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

extern "C" int32_t mm_policy_bank_train_scratch_bytes(int64_t rows, int64_t row_len, int32_t K, const int64_t *col_start,
                                                      uint64_t *bytes) {
  using namespace mm::bank_train;
  Plan P;
  if (!bytes || !plan(rows, row_len, K, col_start, false, P)) return MM_ERR_INVALID_ARG;
  *bytes = (uint64_t)scratch_of(P, K).total * 4u;
  return MM_OK;
}

extern "C" int32_t mm_policy_bank_train(const float *obs, int64_t obs_stride, int64_t rows, int64_t row_len, int32_t n_s,
                                        const int32_t *actions, int64_t act_stride, const float *returns, int64_t ret_stride,
                                        const float *old_logp, const uint8_t *valid, const MMMlpParams *actors,
                                        const MMMlpParams *critics, int32_t K, const int64_t *col_start, int32_t hidden, int32_t n_a,
                                        float clip_param, int32_t critic_loss, int32_t form, const float *advantages,
                                        const float *target_value, const MMMlpParams *actor_grads, const MMMlpParams *critic_grads,
                                        float *loss, float *adv_sums, float *logp_taken, float *value, float *ratio, void *scratch,
                                        uint64_t scratch_bytes, MMStream stream) {
  using namespace mm::bank_train;
  if ((!actors && !critics) || !loss) return MM_ERR_INVALID_ARG;
  if ((actors != nullptr) != (actor_grads != nullptr) || (critics != nullptr) != (critic_grads != nullptr)) return MM_ERR_INVALID_ARG;
  if ((actors && (!complete(actors) || !complete(actor_grads))) || (critics && (!complete(critics) || !complete(critic_grads))))
    return MM_ERR_INVALID_ARG;
  if (critic_loss != MM_PT_CRITIC_MSE && critic_loss != MM_PT_CRITIC_HUBER) return MM_ERR_INVALID_ARG;
  if (form != MM_PT_FORM_REFERENCE && form != MM_PT_FORM_PER_SAMPLE) return MM_ERR_INVALID_ARG;
  if (!(clip_param >= 0.0f)) return MM_ERR_INVALID_ARG;
  if ((!actors && (logp_taken || ratio)) || (!critics && value)) return MM_ERR_INVALID_ARG;
  Plan P;
  if (!plan(rows, row_len, K, col_start, true, P) || !shape_ok(P.n, n_s, hidden, n_a, kHidden)) return MM_ERR_INVALID_ARG;
  const Scratch S = scratch_of(P, K);
  if (P.n > 0) {  // (n == 0: the per-sample inputs and the scratch are not looked at and may be NULL, as in mm_policy_train)
    if (actors && ((advantages != nullptr) == (target_value != nullptr))) return MM_ERR_INVALID_ARG;
    if (!obs || !actions || obs_stride < n_s || (actors && !old_logp) || ((critics || (actors && target_value)) && !returns))
      return MM_ERR_INVALID_ARG;
    if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < (uint64_t)S.total * 4u) return MM_ERR_INVALID_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const int k2c = kHidden + n_a;
  if (hipMemsetAsync(loss, 0, (size_t)K * 2 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
  if (P.n == 0) {  // nothing to contract: zero gradients (K members of each tensor), zero sums
    if (adv_sums && hipMemsetAsync(adv_sums, 0, (size_t)K * 2 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
    if (actors && !zero_mlp_grads(s, actor_grads, kHidden, n_s, kHidden, n_a, K)) return MM_ERR_DEVICE;
    if (critics && !zero_mlp_grads(s, critic_grads, kHidden, n_s, k2c, 1, K)) return MM_ERR_DEVICE;
    return MM_OK;
  }
  float *sc = (float *)scratch;
  int *count = (int *)(sc + S.count);
  float *sums = sc + S.sums;
  double *lossp = (double *)(sc + S.lossp), *stats = (double *)(sc + S.stats);
  const bool ref_form = form == MM_PT_FORM_REFERENCE;
  hipLaunchKernelGGL(bank_frag_kernel, dim3(2 * 4096 / 256, K), dim3(256), 0, s, actors ? actors->W2 : nullptr,
                     critics ? critics->W2 : nullptr, k2c, (float4 *)(sc + S.frag));
  StatArgs st = {};
  st.valid = valid; st.advantages = advantages; st.target_value = target_value; st.returns = returns; st.ret_stride = ret_stride;
  st.sums = actors && ref_form; st.stats = stats;
  const long long stat_blocks = (P.total_tiles + 3) / 4;
  hipLaunchKernelGGL(bank_stats_kernel, dim3((unsigned)(stat_blocks < 2048 ? stat_blocks : 2048)), dim3(256), 0, s, st, P.tb,
                     (int)P.total_tiles);
  hipLaunchKernelGGL(bank_stats_fold_kernel, dim3(K), dim3(256), 0, s, (const double *)stats, P.tb, count, sums, adv_sums);
  SampleArgs a = {};
  a.obs = obs; a.obs_stride = obs_stride; a.n_s = n_s; a.actions = actions; a.act_stride = act_stride; a.returns = returns;
  a.ret_stride = ret_stride; a.old_logp = old_logp; a.valid = valid; a.n_a = n_a; a.clip_param = clip_param;
  a.huber = critic_loss == MM_PT_CRITIC_HUBER; a.ref_form = ref_form; a.adv_sums = sums; a.advantages = advantages;
  a.target_value = target_value; a.count = count;
  a.s_h1 = sc + S.h1; a.s_dz1 = sc + S.dz1; a.s_h2 = sc + S.h2; a.s_dz2 = sc + S.dz2; a.s_dh = sc + S.dh; a.s_xs = sc + S.xs;
  a.lossp = lossp;
  const unsigned grid_a = (unsigned)P.tb.block_start[K], grid_b = (unsigned)P.total_slices;
  for (int net = 0; net < 2; net++) {  // the actors' three kernels, then the critics' over the same scratch
    const MMMlpParams *w = net ? critics : actors;
    if (!w) continue;
    const int k2 = net ? k2c : kHidden, n_out = net ? 1 : n_a;
    a.w = *w; a.frag = (const float4 *)(sc + S.frag + net * kFrag);
    a.out0 = net ? value : logp_taken; a.out1 = net ? nullptr : ratio;
    hipLaunchKernelGGL((net ? bank_sample_kernel<true, true> : bank_sample_kernel<false, true>), dim3(grid_a), dim3(kThreadsA), 0, s, a,
                       P.tb);
    hipLaunchKernelGGL((net ? bank_wgrad_kernel<true> : bank_wgrad_kernel<false>), dim3(grid_b), dim3(kThreadsB), 0, s, a.s_h1, a.s_dz1,
                       a.s_h2, a.s_dz2, a.s_dh, a.s_xs, P.tb, sc + S.part);
    hipLaunchKernelGGL(bank_fold_kernel, dim3((fold_elems(kHidden, n_s, k2, n_out) + 255) / 256 + 1, K), dim3(256), 0, s,
                       (const float *)(sc + S.part), P.tb, (int)n_s, k2, n_out, net ? *critic_grads : *actor_grads,
                       (const double *)lossp, (const int *)count, net ? 0 : (ref_form ? 2 : 1), loss + net);
  }
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
