// mm_policy_gi_bank_train.hip -- K shared actor-critics of one shape, each on its own column group of one batch: the forward
// evaluation (mm_policy_gi_bank_eval) and the loss and full gradient (mm_policy_gi_bank_train) of
// include/mm_policy_gi_bank_train.h.
//
// The arithmetic is mm_policy_gi_train.hip's, from the pieces of mm_policy_mfma.h, and the decomposition of every group is
// mm_policy_gi_train's on that group's n_k samples; what differs is where a tile's inputs and scratch rows live and whose weights
// a workgroup stages.  Kernel A is the text mm_policy_gi_train.hip runs, gi_sample_body of mm_policy_gi_sample.h, with that
// difference as its policy `Group`; kernel B is wgrad_rows and kernel C gi_grad_slot / fold / loss_tree, on the group's own rows,
// partial blocks and tiles.  The group tables, their lookups, the statistics and the plan are mm_policy_bank_train.hip's
// (mm_policy_bank_tables.h).
//
//   frag      W2^T of every member in MFMA A-fragment order (80 KB per member).
//   stats     per 32-sample tile of a group, in fp64: the number of valid samples and the sums of the non-negative and of the
//             negative advantages returns - value_now (a fixed butterfly); stats_fold: one workgroup per group folds its tiles in
//             loss_tree's fixed tree into B_k and the float S+_k, S-_k.
//   kernel A  a workgroup belongs to ONE group (the block prefix table of mm_policy_bank_grid on the n_k): it stages that
//             member's weights once and walks the group's tiles, counted from the group's own start.  Member-local
//             sample i = 32 tile + lane sits at row i / w_k, column col_start[k] + i % w_k of the batch; its scratch rows at
//             32 tile_start[k] + i.  Without the backward it is the evaluation entry's one launch.
//   kernel B  grid = the sum of the groups' slices; a workgroup finds its group from the slice prefix table.
//   kernel C  grid (elements, K): member k folds its own partial blocks in workgroup order, the last workgroup its loss tree.
// The tables ride in the by-value argument blocks (uniform lookups: scalar loads from the kernel-argument segment).
#include "mm_policy_chunked.h"  // gi_grad_slot, gi_elems: policy_gi_train_fold_kernel's index map; mm_policy_mfma.h
#include "mm_policy_gi_sample.h"  // kernel A
#include "mm_policy_bank_tables.h"
#include "../../include/mm_policy_gi_bank_train.h"

namespace mm {
namespace gi_bank_train {

using namespace mfma;
using namespace bank_train;  // Tables, group_of, sample_of, StatArgs, stats_tiles, stats_fold, Plan, plan
constexpr int kWavesA = MM_BANK_WAVES;  // kernel A's 8 waves, as policy_gi_bank_kernel's: mm_policy_bank_grid splits the workgroups
constexpr int kThreadsA = kGiThreadsA;
static_assert(kThreadsA == 64 * kWavesA, "kernel A's workgroup");
constexpr int kThreadsB = 320;
constexpr int kCat = kGiCat;
constexpr long long kFrag = 5 * 4 * 4 * 64 * 4;  // W2^T fragments of one member, in floats
typedef PartialBlock<5> Part;
static_assert(MM_BANK_TILE == 32, "one wave per 32 samples: the MFMA tile");
static_assert(kFrag * 4 == MM_GBT_MEMBER_BYTES && Part::kSize * 4 == MM_GBT_PARTIAL_BYTES, "the header's scratch figures");
static_assert((2 * kCat + 2 * kHidden + kDh + kXs) * 4 == MM_GBT_SAMPLE_BYTES && MM_GBT_TILE_BYTES == (2 + 3) * 8, "the header's scratch figures");
static_assert(MM_GBT_HEADER_BYTES == 4 * 4 * kG && MM_GBT_HEADER_BYTES >= 4 * (kG + 2 * kG), "the header's scratch figures");

// member k of the stacked tensors
MM_DEV MMGiParams member(const MMGiParams &w, int k, int n_a) {
  return {w.W11 + k * 32 * 5, w.b11 + k * 32, w.W12 + k * 64 * 10, w.b12 + k * 64, w.W13 + k * 64 * 10, w.b13 + k * 64,
          w.W2 + k * kHidden * kCat, w.b2 + k * kHidden, w.Wa + k * n_a * kHidden, w.ba + k * n_a, w.Wc + k * kHidden, w.bc + k};
}

// ---- frag: W2^T fragments of member blockIdx.y
__global__ __launch_bounds__(256) void gi_bank_frag_kernel(const float *__restrict__ W2, float4 *__restrict__ frag) {
  const int t = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  frag[(long long)k * (kFrag / 4) + t] = w2t_fragment(W2 + (long long)k * kHidden * kCat, kCat, t);
}

// ---- stats and their fold (mm_policy_bank_tables.h)
__global__ __launch_bounds__(256) void gi_bank_stats_kernel(const StatArgs p, const Tables tb, int total_tiles) {
  stats_tiles(p, tb, total_tiles);
}

__global__ __launch_bounds__(256) void gi_bank_stats_fold_kernel(const double *__restrict__ stats, const Tables tb,
                                                                 int *__restrict__ count, float *__restrict__ sums,
                                                                 float *__restrict__ sums_out) {
  stats_fold(stats, tb, count, sums, sums_out);
}

struct SampleArgs {
  const float *obs;
  long long obs_stride;
  const int32_t *actions;
  long long act_stride;
  const float *returns;
  long long ret_stride;
  const float *old_logp;
  const uint8_t *valid;
  MMGiParams w;  // the twelve stacked bases
  int n_a;
  float clip_param;
  int huber, ref_form;
  const float *adv_sums;  // [K][2]
  const int *count;       // [K]
  const float4 *frag;     // member 0's fragments; member k kFrag floats further
  float *s_h1, *s_dz1, *s_h2, *s_dz2, *s_dh, *s_xs;
  double *lossp;
  float *logp_out, *value_out, *ratio_out;
};

// ---- kernel A: gi_sample_body of mm_policy_gi_sample.h; a workgroup serves the group its index falls in
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
  MM_DEV MMGiParams net() const { return member(p.w, g, p.n_a); }
  MM_DEV const float4 *frag() const { return p.frag + (long long)g * (kFrag / 4); }
  MM_DEV double *lossp() const { return p.lossp + 2 * (row_base >> 5); }
  MM_DEV long long n() const { return n_; }
  MM_DEV long long first_tile(int wave) const { return (long long)lb * kWavesA + wave; }  // tiles are counted from the group's start
  MM_DEV long long tile_stride() const { return (long long)nblk * kWavesA; }
  MM_DEV int count() const { return p.count[g]; }
  MM_DEV const float *adv_sums() const { return p.adv_sums + 2 * g; }
  MM_DEV bool ref_form() const { return p.ref_form != 0; }
  MM_DEV long long sample(long long i, bool in_range) const { return in_range ? (long long)sample_of((unsigned)i, gw, c0, row_len) : 0; }
  MM_DEV long long row(long long i) const { return row_base + i; }
};

template <bool kTrain>
__global__ __launch_bounds__(kThreadsA) void gi_bank_sample_kernel(const SampleArgs a, const Tables tb) {
  gi_sample_body<kTrain>(Group(a, tb));
}

// ---- kernel B: workgroup b = slice b - slice_start[g] of group g
__global__ __launch_bounds__(kThreadsB) void gi_bank_wgrad_kernel(const float *__restrict__ s_h1, const float *__restrict__ s_dz1,
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
  wgrad_rows<5, false>(s_h1, s_dz1, s_h2, s_dz2, s_dh, s_xs, row0, row1, part + (long long)b * Part::kSize);
}

// ---- kernel C: member blockIdx.y; element t = its partial blocks summed in workgroup order (policy_gi_train_fold_kernel's index
// map, gi_grad_slot, on the member's tensors); the last workgroup folds its two losses
__global__ __launch_bounds__(256) void gi_bank_fold_kernel(const float *__restrict__ part_all, const Tables tb, int n_a, MMGiParams gr,
                                                           const double *__restrict__ lossp, const int *__restrict__ count,
                                                           int ref_form, float *__restrict__ loss) {
  const int k = blockIdx.y;
  if (blockIdx.x == gridDim.x - 1) {
    __shared__ double ssum[2][256];  // actor, critic
    const int nt = tb.tile_start[k + 1] - tb.tile_start[k];
    loss_tree<2>(lossp + 2ll * tb.tile_start[k], nt, ssum);
    if (threadIdx.x == 0) {
      const double inv = inv_count(count + k);
      const float a = (float)(-ssum[0][0] * inv * (ref_form ? inv : 1.0)), c = (float)(ssum[1][0] * inv);
      loss[3 * k + 0] = nt > 0 ? a : 0.0f;
      loss[3 * k + 1] = nt > 0 ? c : 0.0f;
      loss[3 * k + 2] = nt > 0 ? a + c : 0.0f;
    }
    return;
  }
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= chunked::gi_elems(n_a)) return;
  const float *part = part_all + (long long)tb.slice_start[k] * Part::kSize;
  const int slices = tb.slice_start[k + 1] - tb.slice_start[k];
  int src;
  float *dst = chunked::gi_grad_slot(t, n_a, member(gr, k, n_a), src);
  *dst = fold<Part::kSize>(part, slices, src);
}

// ---- host side: the scratch, offsets in floats
struct Scratch {
  long long count, sums, frag, h1, dz1, h2, dz2, dh, xs, lossp, stats, part, total;
};

static Scratch scratch_of(const Plan &P, int K) {
  Scratch S;
  const long long n_pad = 32 * P.total_tiles;
  S.count = 0;
  S.sums = kG;
  S.frag = MM_GBT_HEADER_BYTES / 4;
  S.h1 = S.frag + (long long)K * kFrag;
  S.dz1 = S.h1 + n_pad * kCat;
  S.h2 = S.dz1 + n_pad * kCat;
  S.dz2 = S.h2 + n_pad * kHidden;
  S.dh = S.dz2 + n_pad * kHidden;
  S.xs = S.dh + n_pad * kDh;
  S.lossp = S.xs + n_pad * kXs;
  S.stats = S.lossp + 2 * 2 * P.total_tiles;
  S.part = S.stats + 2 * 3 * P.total_tiles;
  S.total = S.part + P.cap_slices * Part::kSize;
  return S;
}

// zeroes the twelve gradient tensors of K stacked members; false: an enqueue failed
static bool zero_grads(hipStream_t s, const MMGiParams &g, int n_a, int K) {
  float *const gp[12] = {g.W11, g.b11, g.W12, g.b12, g.W13, g.b13, g.W2, g.b2, g.Wa, g.ba, g.Wc, g.bc};
  const size_t gsz[12] = {160, 32, 640, 64, 640, 64, (size_t)kHidden * kCat, kHidden, (size_t)n_a * kHidden, (size_t)n_a, kHidden, 1};
  for (int k = 0; k < 12; k++)
    if (hipMemsetAsync(gp[k], 0, gsz[k] * K * sizeof(float), s) != hipSuccess) return false;
  return true;
}

}  // namespace gi_bank_train
}  // namespace mm

extern "C" int32_t mm_policy_gi_bank_eval(const float *obs, int64_t obs_stride, int64_t rows, int64_t row_len, int32_t n_s,
                                          const int32_t *actions, int64_t act_stride, const uint8_t *valid, const MMGiParams *bank,
                                          int32_t K, const int64_t *col_start, int32_t hidden, int32_t n_a, float *logp_taken,
                                          float *value, MMStream stream) {
  using namespace mm::gi_bank_train;
  if (!complete(bank)) return MM_ERR_INVALID_ARG;
  Plan P;
  if (!plan(rows, row_len, K, col_start, true, P) || !shape_ok(P.n, n_s, hidden, n_a, kHidden)) return MM_ERR_INVALID_ARG;
  if (P.n == 0) return MM_OK;  // (the per-sample pointers, the outputs among them, are not looked at)
  if ((!logp_taken && !value) || !obs || !actions || obs_stride < n_s) return MM_ERR_INVALID_ARG;
  SampleArgs a = {};
  a.obs = obs; a.obs_stride = obs_stride; a.actions = actions; a.act_stride = act_stride; a.valid = valid; a.w = *bank; a.n_a = n_a;
  a.logp_out = logp_taken; a.value_out = value;
  hipLaunchKernelGGL(gi_bank_sample_kernel<false>, dim3((unsigned)P.tb.block_start[K]), dim3(kThreadsA), 0, (hipStream_t)stream, a,
                     P.tb);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

extern "C" int32_t mm_policy_gi_bank_train_scratch_bytes(int64_t rows, int64_t row_len, int32_t K, const int64_t *col_start,
                                                         uint64_t *bytes) {
  using namespace mm::gi_bank_train;
  Plan P;
  if (!bytes || !plan(rows, row_len, K, col_start, false, P)) return MM_ERR_INVALID_ARG;
  *bytes = (uint64_t)scratch_of(P, K).total * 4u;
  return MM_OK;
}

extern "C" int32_t mm_policy_gi_bank_train(const float *obs, int64_t obs_stride, int64_t rows, int64_t row_len, int32_t n_s,
                                           const int32_t *actions, int64_t act_stride, const float *returns, int64_t ret_stride,
                                           const float *old_logp, const uint8_t *valid, const MMGiParams *bank, int32_t K,
                                           const int64_t *col_start, int32_t hidden, int32_t n_a, float clip_param,
                                           int32_t critic_loss, int32_t form, const float *value_now, const MMGiParams *grads,
                                           float *loss, float *adv_sums, float *logp_taken, float *value, float *ratio, void *scratch,
                                           uint64_t scratch_bytes, MMStream stream) {
  using namespace mm::gi_bank_train;
  if (!complete(bank) || !complete(grads) || !loss) return MM_ERR_INVALID_ARG;
  if (critic_loss != MM_GI_CRITIC_MSE && critic_loss != MM_GI_CRITIC_HUBER) return MM_ERR_INVALID_ARG;
  if (form != MM_PT_FORM_REFERENCE && form != MM_PT_FORM_PER_SAMPLE) return MM_ERR_INVALID_ARG;
  if (!(clip_param >= 0.0f)) return MM_ERR_INVALID_ARG;
  Plan P;
  if (!plan(rows, row_len, K, col_start, true, P) || !shape_ok(P.n, n_s, hidden, n_a, kHidden)) return MM_ERR_INVALID_ARG;
  const Scratch S = scratch_of(P, K);
  const bool ref_form = form == MM_PT_FORM_REFERENCE;
  if (P.n > 0) {  // (n == 0: the per-sample inputs and the scratch are not looked at and may be NULL, as in mm_policy_gi_train)
    if (!obs || !actions || !returns || !old_logp || obs_stride < n_s) return MM_ERR_INVALID_ARG;
    if (ref_form != (value_now != nullptr)) return MM_ERR_INVALID_ARG;
    if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < (uint64_t)S.total * 4u) return MM_ERR_INVALID_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  if (P.n == 0) {  // nothing to contract: zero gradients (K members of each tensor), zero losses and sums
    if (hipMemsetAsync(loss, 0, (size_t)K * 3 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
    if (adv_sums && hipMemsetAsync(adv_sums, 0, (size_t)K * 2 * sizeof(float), s) != hipSuccess) return MM_ERR_DEVICE;
    return zero_grads(s, *grads, n_a, K) ? MM_OK : MM_ERR_DEVICE;
  }
  float *sc = (float *)scratch;
  int *count = (int *)(sc + S.count);
  float *sums = sc + S.sums;
  double *lossp = (double *)(sc + S.lossp), *stats = (double *)(sc + S.stats);
  hipLaunchKernelGGL(gi_bank_frag_kernel, dim3((unsigned)(kFrag / 4 / 256), K), dim3(256), 0, s, (const float *)bank->W2,
                     (float4 *)(sc + S.frag));
  StatArgs st = {};
  st.valid = valid; st.target_value = value_now; st.returns = returns; st.ret_stride = ret_stride; st.sums = ref_form; st.stats = stats;
  const long long stat_blocks = (P.total_tiles + 3) / 4;
  hipLaunchKernelGGL(gi_bank_stats_kernel, dim3((unsigned)(stat_blocks < 2048 ? stat_blocks : 2048)), dim3(256), 0, s, st, P.tb,
                     (int)P.total_tiles);
  hipLaunchKernelGGL(gi_bank_stats_fold_kernel, dim3(K), dim3(256), 0, s, (const double *)stats, P.tb, count, sums, adv_sums);
  SampleArgs a = {};
  a.obs = obs; a.obs_stride = obs_stride; a.actions = actions; a.act_stride = act_stride; a.returns = returns; a.ret_stride = ret_stride;
  a.old_logp = old_logp; a.valid = valid; a.w = *bank; a.n_a = n_a; a.clip_param = clip_param;
  a.huber = critic_loss == MM_GI_CRITIC_HUBER; a.ref_form = ref_form; a.adv_sums = sums; a.count = count;
  a.frag = (const float4 *)(sc + S.frag);
  a.s_h1 = sc + S.h1; a.s_dz1 = sc + S.dz1; a.s_h2 = sc + S.h2; a.s_dz2 = sc + S.dz2; a.s_dh = sc + S.dh; a.s_xs = sc + S.xs;
  a.lossp = lossp; a.logp_out = logp_taken; a.value_out = value; a.ratio_out = ratio;
  hipLaunchKernelGGL(gi_bank_sample_kernel<true>, dim3((unsigned)P.tb.block_start[K]), dim3(kThreadsA), 0, s, a, P.tb);
  hipLaunchKernelGGL(gi_bank_wgrad_kernel, dim3((unsigned)P.total_slices), dim3(kThreadsB), 0, s, (const float *)a.s_h1,
                     (const float *)a.s_dz1, (const float *)a.s_h2, (const float *)a.s_dz2, (const float *)a.s_dh,
                     (const float *)a.s_xs, P.tb, sc + S.part);
  hipLaunchKernelGGL(gi_bank_fold_kernel, dim3((unsigned)((mm::chunked::gi_elems(n_a) + 255) / 256 + 1), K), dim3(256), 0, s,
                     (const float *)(sc + S.part), P.tb, (int)n_a, *grads, (const double *)lossp, (const int *)count, (int)ref_form,
                     loss);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
