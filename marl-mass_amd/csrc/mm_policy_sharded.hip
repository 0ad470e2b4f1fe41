// mm_policy_sharded.hip -- one gradient over a batch that is sharded over ranks, in two phases: mm_policy_gi_train_partial /
// mm_policy_gi_train_finish (include/mm_policy_gi_train.h), mm_policy_train_partial / mm_policy_train_finish
// (include/mm_policy_train.h) and, at hidden 512, mm_policy_wide_train_partial / mm_policy_wide_train_finish
// (include/mm_policy_wide_train.h).
//
// The chunked entries (mm_policy_chunked.hip) already work in stages: kernels A and B in passes, every pass's partial blocks added
// into an fp64 accumulator block per network, one finish kernel that rounds the block to float32 in torch layout.  Here the
// accumulator is the caller's: `partial` runs the same prep and the same passes on the rank's own samples -- the chunked entries'
// own pass loops and argument checks (mm_policy_chunked.h), kernel A scaled by the count B of the WHOLE batch, which the caller
// gives -- and leaves a shard block
//
//   [0] B   [1] the rank's own count of valid samples   [2] the configuration word   [3] 0
//   [4] [5] the un-normalised fp64 loss sums (shared network: actor, critic heads; separate networks: actor, critic)
//   [6 ..)  the accumulator block(s): PartialBlock<5> (shared network) | F::Part actor, F::Part critic (separate networks:
//           PartialBlock<4>, 26 896 doubles, at hidden 128; wt::Part, 304 144 doubles, at hidden 512)
//
// and `finish` folds R of them: one thread per gradient element starts from block 0's value, adds blocks 1 .. R - 1 in index
// order in fp64, rounds once to float32 and writes it through the index maps of the chunked finish kernels; the last workgroup
// adds the R loss doubles in index order and scales them with the chunked finish's expression.  With R = 1 and B the rank's own
// count every one of these steps is the chunked entry's, so the results are its bits.
//
// The accumulate kernel walks whole partial blocks, slots no kernel B writes included, and adds whatever the scratch held
// there.  A shard block is gathered over ranks and visible to the caller, so the tail kernel of the separate networks' `partial`
// writes 0.0 into every accumulator slot that the finish index map does not read for the call's n_s and n_a (dW2 columns from k2
// on, head rows and head bias from n_out on, dW1 columns from n_s on): every double of the block is a function of the inputs.
//
// finish cannot refuse on the host what is wrong on the device, so every wave first reads the R headers: every block must carry
// the same B and configuration word, the word must be that of the call (n_s, n_a, and hidden 512 there) and name every requested
// network, and the local counts must add up to B.  If not, every requested gradient and every loss is written as NaN.  B == 0
// writes zeros.  No floating-point atomics; only enqueues on the stream.
//
// The separate actor and critic are written once for both hidden sizes, against the traits Pt128 and Pt512 (mm_policy_chunked.h).
#include <type_traits>

#include "mm_policy_chunked.h"

namespace mm {
namespace sharded {

using namespace mfma;
using namespace chunked;

constexpr int kHeader = 4, kLoss = 2, kAcc = kHeader + kLoss;  // doubles
constexpr long long kGiDoubles = kAcc + PartGi::kSize;
template <class F>
constexpr long long kPtDoubles = kAcc + 2ll * F::Part::kSize;
static_assert(kGiDoubles == MM_GI_SHARD_DOUBLES && kPtDoubles<Pt128> == MM_PT_SHARD_DOUBLES && kPtDoubles<Pt512> == MM_PW_SHARD_DOUBLES,
              "the shard blocks of the public headers");
constexpr int kNetActor = 1, kNetCritic = 2;  // the configuration word's networks (the shared network is both)

// n_s + 2^8 n_a + 2^16 (reference form + 2 huber) + 2^24 networks + wide_bit (2^26 at hidden 512, else 0): an integer below 2^31,
// exact in a double
static double config_word(int n_s, int n_a, bool ref_form, bool huber, int nets, int wide_bit) {
  return (double)(n_s + 256 * n_a + 65536 * ((ref_form ? 1 : 0) + (huber ? 2 : 0)) + 16777216 * nets + wide_bit);
}

MM_DEV void write_header(double *shard, const int *count, const int *local, double config) {
  shard[0] = (double)*count;
  shard[1] = local ? (double)*local : 0.0;
  shard[2] = config;
  shard[3] = 0.0;
}

// ---- the end of `partial`, shared network: the rank's loss partials, both sums per tile, folded with the chunked finish's tree
// (ntiles 0: an empty shard), and the header.  One workgroup.
__global__ __launch_bounds__(256) void train_shard_header_kernel(const double *__restrict__ lossp, long long ntiles,
                                                                 const int *__restrict__ count, const int *__restrict__ local,
                                                                 double config, double *__restrict__ shard) {
  __shared__ double ssum[2][256];
  loss_tree<2>(lossp, ntiles, ssum);
  if (threadIdx.x != 0) return;
  shard[kHeader] = ssum[0][0];
  shard[kHeader + 1] = ssum[1][0];
  write_header(shard, count, local, config);
}

// ---- the end of `partial`, separate networks.  Workgroup k < 2 folds network k's loss partials with the chunked finish's tree
// (NULL: the network is not there and its sum stays the memset's zero); workgroup 0 also writes the header.  The workgroups from 2
// on scrub: one thread per accumulator slot of the two blocks, consecutive threads on consecutive doubles, 0.0 where finish does
// not read.
template <class F>
__global__ __launch_bounds__(256) void train_shard_tail_kernel(const double *__restrict__ lossp0, const double *__restrict__ lossp1,
                                                               long long ntiles, const int *__restrict__ count,
                                                               const int *__restrict__ local, double config, int n_s, int n_a,
                                                               double *__restrict__ shard) {
  typedef typename F::Part Part;
  if (blockIdx.x >= 2) {
    int off = (blockIdx.x - 2) * 256 + threadIdx.x;
    if (off >= 2 * Part::kSize) return;
    const bool critic = off >= Part::kSize;
    if (critic) off -= Part::kSize;
    if (!slot_is_read<F>(off, n_s, critic ? F::kHid + n_a : F::kHid, critic ? 1 : n_a)) shard[kAcc + (critic ? Part::kSize : 0) + off] = 0.0;
    return;
  }
  __shared__ double ssum[1][256];
  const double *lp = blockIdx.x ? lossp1 : lossp0;
  if (lp) {
    loss_tree<1>(lp, ntiles, ssum);
    if (threadIdx.x == 0) shard[kHeader + blockIdx.x] = ssum[0][0];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) write_header(shard, count, local, config);
}

// ---- finish
struct FinishArgs {
  const double *blocks;
  long long stride;  // doubles from one block to the next
  int n_blocks, n_s, n_a, want;  // want: the networks whose gradients are written
  int nelem_a, nelem_c;          // gradient elements of the first / second requested network (0: not requested)
  MMGiParams gi;
  MMMlpParams actor, critic;
  float *loss;
};

// What the R headers say, computed by every wave alone (lane r reads block r): 0 = inconsistent, 1 = consistent.
MM_DEV int shard_headers(const FinishArgs &a, int wide_bit, double &b_out, int &mode) {
  const int lane = threadIdx.x & 63;
  const double b0 = a.blocks[0], w0 = a.blocks[2];
  double c = 0.0;
  bool bad = false;
  if (lane < a.n_blocks) {
    const double *h = a.blocks + lane * a.stride;
    c = h[1];
    bad = h[0] != b0 || h[2] != w0 || !(c >= 0.0 && c <= 2147483647.0);
    if (bad) c = 0.0;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);  // (integers below 2^37: exact in any order)
  bad = __ballot(bad) != 0;
  if (!(b0 >= 0.0 && b0 <= 2147483647.0) || !(w0 >= 0.0 && w0 < 2147483648.0)) bad = true;
  const int w = bad ? 0 : (int)w0;
  if ((double)w != w0 || (double)(int)(bad ? 0.0 : b0) != b0) bad = true;
  if ((w & 255) != a.n_s || ((w >> 8) & 255) != a.n_a || ((w >> 24) & a.want) != a.want || (w & wide_bit) != wide_bit) bad = true;
  if (c != b0) bad = true;
  b_out = b0;
  mode = (w >> 16) & 255;
  return bad ? 0 : 1;
}

// the shared network in F's place: its own index map and a third loss, the rest is the separate networks' at hidden 128
struct Gi {
  static constexpr int kWideBit = 0;
};

template <class F>
__global__ __launch_bounds__(256) void train_shard_finish_kernel(const FinishArgs a) {
  constexpr bool kShared = std::is_same<F, Gi>::value;
  double b;
  int mode;
  const int ok = shard_headers(a, F::kWideBit, b, mode);
  const float nan = __builtin_nanf("");
  if (blockIdx.x == gridDim.x - 1) {
    if (threadIdx.x != 0) return;
    double s[kLoss];
#pragma unroll
    for (int k = 0; k < kLoss; k++) s[k] = a.blocks[kHeader + k];
    for (int r = 1; r < a.n_blocks; r++) {
#pragma unroll
      for (int k = 0; k < kLoss; k++) s[k] += a.blocks[r * a.stride + kHeader + k];
    }
    const int nb = (int)b;
    const double inv = nb > 0 ? 1.0 / (double)nb : 0.0;
    const bool ref = mode & 1;
    const float la = (a.want & kNetActor) ? (float)(ref ? -s[0] * inv * inv : -s[0] * inv) : 0.0f;
    const float lc = (a.want & kNetCritic) ? (float)(s[1] * inv) : 0.0f;
    a.loss[0] = ok ? la : nan;
    a.loss[1] = ok ? lc : nan;
    if constexpr (kShared) a.loss[2] = ok ? la + lc : nan;
    return;
  }
  int t = blockIdx.x * 256 + threadIdx.x, src;
  float *dst;
  if constexpr (kShared) {
    if (t >= a.nelem_a) return;
    dst = gi_grad_slot(t, a.n_a, a.gi, src);
  } else if (t < a.nelem_a) {
    dst = grad_slot<F>(t, a.n_s, F::kHid, a.n_a, a.actor, src);
  } else {
    t -= a.nelem_a;
    if (t >= a.nelem_c) return;
    dst = grad_slot<F>(t, a.n_s, F::kHid + a.n_a, 1, a.critic, src);
    src += F::Part::kSize;
  }
  if (!dst) return;
  float out = nan;
  if (ok) {
    const double *p = a.blocks + kAcc + src;
    double sum = p[0];
#pragma unroll 4
    for (int r = 1; r < a.n_blocks; r++) sum += p[r * a.stride];
    out = b > 0.0 ? (float)sum : 0.0f;
  }
  *dst = out;
}

static bool aligned(const void *p, uintptr_t to) { return p && !((uintptr_t)p & (to - 1)); }

// what every finish entry refuses alike, besides its gradients: the blocks, their number and stride, the shape
static bool finish_args_ok(const double *blocks, int32_t n_blocks, int64_t stride, long long doubles, int32_t n_s, int32_t n_a,
                           const float *loss) {
  return loss && aligned(blocks, 8) && n_blocks >= 1 && n_blocks <= 64 && stride >= doubles && n_s >= 25 && n_s <= 32 && n_a >= 1 &&
         n_a <= 8;
}

template <class F>
static int launch_finish(hipStream_t s, FinishArgs &a, const double *blocks, int32_t n_blocks, int64_t stride, float *loss) {
  a.blocks = blocks; a.stride = stride; a.n_blocks = n_blocks; a.loss = loss;
  hipLaunchKernelGGL(train_shard_finish_kernel<F>, dim3((a.nelem_a + a.nelem_c + 255) / 256 + 1), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

static int32_t shard_bytes(long long doubles, uint64_t *bytes) {
  if (!bytes) return MM_ERR_INVALID_ARG;
  *bytes = (uint64_t)doubles * sizeof(double);
  return MM_OK;
}

// ---- the separate networks' two entries at hidden F::kHid
template <class F>
static int32_t train_partial(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions, int64_t act_stride,
                             const float *returns, int64_t ret_stride, const float *old_logp, const uint8_t *valid,
                             const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden, int32_t n_a, float clip_param,
                             int32_t critic_loss, const float *adv_sums, const float *advantages, const int32_t *count, double *shard,
                             float *logp_taken, float *value, float *ratio, void *scratch, uint64_t scratch_bytes, MMStream stream,
                             int64_t chunk) {
  typedef typename F::Part Part;
  // everything that can refuse the call comes before the first enqueue
  if (!aligned(count, 4) || !aligned(shard, 16)) return MM_ERR_INVALID_ARG;
  float *sc = (float *)scratch;
  int *local = (int *)sc;  // prep's count: the rank's own
  typename F::PassArgs p = {};  // the rank's samples
  p.obs = obs; p.obs_stride = obs_stride; p.n = n; p.n_s = n_s; p.actions = actions; p.act_stride = act_stride; p.returns = returns;
  p.ret_stride = ret_stride; p.old_logp = old_logp; p.valid = valid; p.n_a = n_a; p.clip_param = clip_param;
  p.huber = critic_loss == MM_PT_CRITIC_HUBER; p.adv_sums = adv_sums; p.advantages = advantages; p.count = count;  // (the WHOLE batch's B)
  const Net net[2] = {{actor, logp_taken, ratio}, {critic, value, nullptr}};
  ChunkLayout<typename F::Layout> L;
  if (!args_ok<F>(p, net, hidden, critic_loss, chunk, scratch, scratch_bytes, L)) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const double config =
      config_word(n_s, n_a, actor && adv_sums, p.huber, (actor ? kNetActor : 0) | (critic ? kNetCritic : 0), F::kWideBit);
  if (hipMemsetAsync(shard, 0, kPtDoubles<F> * sizeof(double), s) != hipSuccess) return MM_ERR_DEVICE;
  if (n == 0) {  // an empty shard: a valid all-zero block with local count 0
    hipLaunchKernelGGL(train_shard_tail_kernel<F>, dim3(1), dim3(256), 0, s, (const double *)nullptr, (const double *)nullptr, 0ll,
                       (const int *)count, (const int *)nullptr, config, (int)n_s, (int)n_a, shard);
    return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
  }
  const double *lossp = (const double *)(sc + L.lossp);  // the actor's, then the critic's
  if (hipMemsetAsync(local, 0, sizeof(int), s) != hipSuccess) return MM_ERR_DEVICE;
  passes<F>(s, p, net, chunk, L, sc, shard + kAcc);
  hipLaunchKernelGGL(train_shard_tail_kernel<F>, dim3(2 + (2 * Part::kSize + 255) / 256), dim3(256), 0, s, actor ? lossp : nullptr,
                     critic ? lossp + L.ntiles : nullptr, L.ntiles, (const int *)count, (const int *)local, config, (int)n_s, (int)n_a,
                     shard);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

template <class F>
static int32_t train_finish(const double *blocks, int32_t n_blocks, int64_t block_stride, int32_t n_s, int32_t n_a,
                            const MMMlpParams *actor_grads, const MMMlpParams *critic_grads, float *loss, MMStream stream) {
  if ((!actor_grads && !critic_grads) || !finish_args_ok(blocks, n_blocks, block_stride, kPtDoubles<F>, n_s, n_a, loss)) return MM_ERR_INVALID_ARG;
  if ((actor_grads && !complete(actor_grads)) || (critic_grads && !complete(critic_grads))) return MM_ERR_INVALID_ARG;
  FinishArgs a = {};
  a.n_s = n_s; a.n_a = n_a;
  if (actor_grads) { a.want |= kNetActor; a.nelem_a = grad_elems<F>(n_s, F::kHid, n_a); a.actor = *actor_grads; }
  if (critic_grads) { a.want |= kNetCritic; a.nelem_c = grad_elems<F>(n_s, F::kHid + n_a, 1); a.critic = *critic_grads; }
  return launch_finish<F>((hipStream_t)stream, a, blocks, n_blocks, block_stride, loss);
}

}  // namespace sharded
}  // namespace mm

extern "C" int32_t mm_policy_gi_train_shard_bytes(uint64_t *bytes) { return mm::sharded::shard_bytes(mm::sharded::kGiDoubles, bytes); }

extern "C" int32_t mm_policy_train_shard_bytes(uint64_t *bytes) {
  return mm::sharded::shard_bytes(mm::sharded::kPtDoubles<mm::chunked::Pt128>, bytes);
}

extern "C" int32_t mm_policy_wide_train_shard_bytes(uint64_t *bytes) {
  return mm::sharded::shard_bytes(mm::sharded::kPtDoubles<mm::chunked::Pt512>, bytes);
}

extern "C" int32_t mm_policy_gi_train_partial(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                              int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                              const uint8_t *valid, const MMGiParams *weights, int32_t hidden, int32_t n_a,
                                              float clip_param, int32_t critic_loss, const float *adv_sums, const int32_t *count,
                                              double *shard, float *logp_taken, float *value, float *ratio, void *scratch,
                                              uint64_t scratch_bytes, MMStream stream, int64_t chunk) {
  using namespace mm::sharded;
  // everything that can refuse the call comes before the first enqueue
  if (!weights || !aligned(count, 4) || !aligned(shard, 16)) return MM_ERR_INVALID_ARG;
  float *sc = (float *)scratch;
  int *local = (int *)sc;  // prep's count: the rank's own
  mm::gi_train::PassArgs p = {};  // the rank's samples
  p.obs = obs; p.obs_stride = obs_stride; p.n = n; p.actions = actions; p.act_stride = act_stride; p.returns = returns;
  p.ret_stride = ret_stride; p.old_logp = old_logp; p.valid = valid; p.w = *weights; p.n_a = n_a; p.clip_param = clip_param;
  p.huber = critic_loss == MM_GI_CRITIC_HUBER; p.adv_sums = adv_sums; p.count = count;  // (kernel A scales by the WHOLE batch's B)
  p.logp_out = logp_taken; p.value_out = value; p.ratio_out = ratio;
  ChunkLayout<Layout> L;
  if (!gi_args_ok(p, n_s, hidden, critic_loss, chunk, scratch, scratch_bytes, L)) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const double config = config_word(n_s, n_a, adv_sums != nullptr, p.huber, kNetActor | kNetCritic, 0);
  if (hipMemsetAsync(shard, 0, kGiDoubles * sizeof(double), s) != hipSuccess) return MM_ERR_DEVICE;
  if (n == 0) {  // an empty shard: a valid all-zero block with local count 0
    hipLaunchKernelGGL(train_shard_header_kernel, dim3(1), dim3(256), 0, s, (const double *)nullptr, 0ll, (const int *)count,
                       (const int *)nullptr, config, shard);
    return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
  }
  if (hipMemsetAsync(local, 0, sizeof(int), s) != hipSuccess) return MM_ERR_DEVICE;
  gi_passes(s, p, chunk, L, sc, shard + kAcc);
  hipLaunchKernelGGL(train_shard_header_kernel, dim3(1), dim3(256), 0, s, (const double *)(sc + L.lossp), L.ntiles, (const int *)count,
                     (const int *)local, config, shard);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

extern "C" int32_t mm_policy_gi_train_finish(const double *blocks, int32_t n_blocks, int64_t block_stride, int32_t n_s, int32_t n_a,
                                             const MMGiParams *grads, float *loss, MMStream stream) {
  using namespace mm::sharded;
  if (!complete(grads) || !finish_args_ok(blocks, n_blocks, block_stride, kGiDoubles, n_s, n_a, loss)) return MM_ERR_INVALID_ARG;
  FinishArgs a = {};
  a.n_s = n_s; a.n_a = n_a; a.want = kNetActor | kNetCritic; a.nelem_a = gi_elems(n_a); a.gi = *grads;
  return launch_finish<Gi>((hipStream_t)stream, a, blocks, n_blocks, block_stride, loss);
}

extern "C" int32_t mm_policy_train_partial(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                           int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                           const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden,
                                           int32_t n_a, float clip_param, int32_t critic_loss, const float *adv_sums,
                                           const float *advantages, const int32_t *count, double *shard, float *logp_taken, float *value,
                                           float *ratio, void *scratch, uint64_t scratch_bytes, MMStream stream, int64_t chunk) {
  return mm::sharded::train_partial<mm::chunked::Pt128>(obs, obs_stride, n, n_s, actions, act_stride, returns, ret_stride, old_logp, valid,
                                                        actor, critic, hidden, n_a, clip_param, critic_loss, adv_sums, advantages, count,
                                                        shard, logp_taken, value, ratio, scratch, scratch_bytes, stream, chunk);
}

extern "C" int32_t mm_policy_train_finish(const double *blocks, int32_t n_blocks, int64_t block_stride, int32_t n_s, int32_t n_a,
                                          const MMMlpParams *actor_grads, const MMMlpParams *critic_grads, float *loss, MMStream stream) {
  return mm::sharded::train_finish<mm::chunked::Pt128>(blocks, n_blocks, block_stride, n_s, n_a, actor_grads, critic_grads, loss, stream);
}

extern "C" int32_t mm_policy_wide_train_partial(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                                int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                                const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden,
                                                int32_t n_a, float clip_param, int32_t critic_loss, const float *adv_sums,
                                                const float *advantages, const int32_t *count, double *shard, float *logp_taken, float *value,
                                                float *ratio, void *scratch, uint64_t scratch_bytes, MMStream stream, int64_t chunk) {
  return mm::sharded::train_partial<mm::chunked::Pt512>(obs, obs_stride, n, n_s, actions, act_stride, returns, ret_stride, old_logp, valid,
                                                        actor, critic, hidden, n_a, clip_param, critic_loss, adv_sums, advantages, count,
                                                        shard, logp_taken, value, ratio, scratch, scratch_bytes, stream, chunk);
}

extern "C" int32_t mm_policy_wide_train_finish(const double *blocks, int32_t n_blocks, int64_t block_stride, int32_t n_s, int32_t n_a,
                                               const MMMlpParams *actor_grads, const MMMlpParams *critic_grads, float *loss, MMStream stream) {
  return mm::sharded::train_finish<mm::chunked::Pt512>(blocks, n_blocks, block_stride, n_s, n_a, actor_grads, critic_grads, loss, stream);
}
