// mm_policy_wide_sharded.hip -- the hidden-512 gradient over a batch that is sharded over ranks, in two phases:
// mm_policy_wide_train_partial / mm_policy_wide_train_finish (include/mm_policy_wide_train.h).
//
// mm_policy_sharded.hip's design at hidden 512.  The chunked entry (mm_policy_wide_chunked.hip) works in stages: kernels A and B
// in passes, every pass's partial blocks added into an fp64 accumulator block per network, one finish kernel per network that
// rounds the block to float32 in torch layout.  Here the accumulator is the caller's: `partial` runs the same prep and the same
// passes on the rank's own samples -- the chunked entry's own pass loop and argument check (mm_policy_wide_chunked.h), kernel A
// scaled by the count B of the WHOLE batch, which the caller gives -- and leaves a shard block
//
//   [0] B   [1] the rank's own count of valid samples   [2] the configuration word (with the hidden-512 bit)   [3] 0
//   [4] [5] the un-normalised fp64 loss sums of the actor and of the critic
//   [6 ..)  the actor's accumulator block (wt::Part, 304 144 doubles), then the critic's
//
// and `finish` folds R of them: one thread per gradient element starts from block 0's value, adds blocks 1 .. R - 1 in index
// order in fp64, rounds once to float32 and writes it through the index map of policy_wide_chunked_finish_kernel; the last
// workgroup adds the R loss doubles in index order and scales them with the chunked finish's expressions.  With R = 1 and B the
// rank's own count every one of these steps is the chunked entry's, so the results are its bits.
//
// The accumulate kernel walks whole partial blocks, slots no kernel B writes included, and adds whatever the scratch held
// there.  A shard block is gathered over ranks and visible to the caller, so the tail kernel of `partial` writes 0.0 into every
// accumulator slot that the finish index map does not read for the call's n_s and n_a (dW2 columns from k2 on, head rows and
// head bias from n_out on, dW1 columns from n_s on): every double of the block is a function of the inputs.
//
// finish cannot refuse on the host what is wrong on the device, so every wave first reads the R headers: every block must carry
// the same B and configuration word, the word must be that of the call (n_s, n_a, hidden 512) and name every requested network,
// and the local counts must add up to B.  If not, every requested gradient and both losses are written as NaN.  B == 0 writes
// zeros.  No floating-point atomics; only enqueues on the stream.
#include "mm_policy_wide_chunked.h"

namespace mm {
namespace wide_sharded {

using namespace mfma;
using namespace wide_chunked;
using wt::kCat;
using wt::kWide;
typedef wt::Part Part;

constexpr int kHeader = 4, kLoss = 2, kAcc = kHeader + kLoss;  // doubles
constexpr long long kDoubles = kAcc + 2ll * Part::kSize;
static_assert(kDoubles == MM_PW_SHARD_DOUBLES, "the shard block of the public header");
constexpr int kNetActor = 1, kNetCritic = 2;  // the configuration word's networks
constexpr int kWideBit = 1 << 26;             // the configuration word's "hidden 512"

// n_s + 2^8 n_a + 2^16 (reference form + 2 huber) + 2^24 networks + 2^26: an integer below 2^31, exact in a double
static double config_word(int n_s, int n_a, bool ref_form, bool huber, int nets) {
  return (double)(n_s + 256 * n_a + 65536 * ((ref_form ? 1 : 0) + (huber ? 2 : 0)) + 16777216 * nets + kWideBit);
}

// whether the finish index map reads slot `off` of the accumulator of a network with fc2 rows of k2 floats and n_out outputs
MM_DEV bool slot_is_read(int off, int n_s, int k2, int n_out) {
  if (off < Part::kHd) return off % kCat < k2;
  if (off < Part::kW1) return off - Part::kHd < n_out * kWide;
  if (off < Part::kb2) return (off - Part::kW1) % 32 < n_s;
  if (off < Part::kbh) return true;
  if (off < Part::kb1) return off - Part::kbh < n_out;
  return true;
}

// ---- the end of `partial`.  Workgroup k < 2 folds network k's loss partials with the chunked finish's tree (NULL: the network
// is not there and its sum stays the memset's zero); workgroup 0 also writes the header.  The workgroups from 2 on scrub: one
// thread per accumulator slot of the two blocks, consecutive threads on consecutive doubles, 0.0 where finish does not read.
__global__ __launch_bounds__(256) void wide_shard_tail_kernel(const double *__restrict__ lossp0, const double *__restrict__ lossp1,
                                                              long long ntiles, const int *__restrict__ count,
                                                              const int *__restrict__ local, double config, int n_s, int n_a,
                                                              double *__restrict__ shard) {
  if (blockIdx.x >= 2) {
    int off = (blockIdx.x - 2) * 256 + threadIdx.x;
    if (off >= 2 * Part::kSize) return;
    const bool critic = off >= Part::kSize;
    if (critic) off -= Part::kSize;
    if (!slot_is_read(off, n_s, critic ? kWide + n_a : kWide, critic ? 1 : n_a)) shard[kAcc + (critic ? Part::kSize : 0) + off] = 0.0;
    return;
  }
  __shared__ double ssum[1][256];
  const double *lp = blockIdx.x ? lossp1 : lossp0;
  if (lp) {
    loss_tree<1>(lp, ntiles, ssum);
    if (threadIdx.x == 0) shard[kHeader + blockIdx.x] = ssum[0][0];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    shard[0] = (double)*count;
    shard[1] = local ? (double)*local : 0.0;
    shard[2] = config;
    shard[3] = 0.0;
  }
}

// ---- finish
struct FinishArgs {
  const double *blocks;
  long long stride;  // doubles from one block to the next
  int n_blocks, n_s, n_a, want;  // want: the networks whose gradients are written
  int nelem_a, nelem_c;          // gradient elements of the actor / the critic (0: not requested)
  MMMlpParams actor, critic;
  float *loss;
};

__host__ __device__ inline int wide_elems(int n_s, int k2, int n_out) {
  return kWide * n_s + kWide + kWide * k2 + kWide + n_out * kWide + n_out;
}

// policy_wide_chunked_finish_kernel's index map (mm_policy_wide_chunked.hip) for a network with fc2 rows of k2 floats and n_out
// outputs: element t of its six gradients -> where it is written (nullptr past the last element); src: its accumulator slot
MM_DEV float *wide_grad_slot(int t, int n_s, int k2, int n_out, const MMMlpParams &gr, int &src) {
  if (t < kWide * n_s) { const int o = t / n_s, k = t % n_s; src = Part::kW1 + o * 32 + k; return gr.W1 + t; }
  t -= kWide * n_s;
  if (t < kWide) { src = Part::kb1 + t; return gr.b1 + t; }
  t -= kWide;
  if (t < kWide * k2) { const int o = t / k2, k = t % k2; src = Part::kW2 + o * kCat + k; return gr.W2 + t; }
  t -= kWide * k2;
  if (t < kWide) { src = Part::kb2 + t; return gr.b2 + t; }
  t -= kWide;
  if (t < n_out * kWide) { src = Part::kHd + t; return gr.W3 + t; }
  t -= n_out * kWide;
  src = Part::kbh + t;
  return t < n_out ? gr.b3 + t : nullptr;
}

// What the R headers say, computed by every wave alone (lane r reads block r): 0 = inconsistent, 1 = consistent.
MM_DEV int shard_headers(const FinishArgs &a, double &b_out, int &mode) {
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
  if ((w & 255) != a.n_s || ((w >> 8) & 255) != a.n_a || ((w >> 24) & a.want) != a.want || !(w & kWideBit)) bad = true;
  if (c != b0) bad = true;
  b_out = b0;
  mode = (w >> 16) & 255;
  return bad ? 0 : 1;
}

__global__ __launch_bounds__(256) void wide_shard_finish_kernel(const FinishArgs a) {
  double b;
  int mode;
  const int ok = shard_headers(a, b, mode);
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
    return;
  }
  int t = blockIdx.x * 256 + threadIdx.x, src;
  float *dst;
  if (t < a.nelem_a) {
    dst = wide_grad_slot(t, a.n_s, kWide, a.n_a, a.actor, src);
  } else {
    t -= a.nelem_a;
    if (t >= a.nelem_c) return;
    dst = wide_grad_slot(t, a.n_s, kWide + a.n_a, 1, a.critic, src);
    src += Part::kSize;
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

}  // namespace wide_sharded
}  // namespace mm

extern "C" int32_t mm_policy_wide_train_shard_bytes(uint64_t *bytes) {
  if (!bytes) return MM_ERR_INVALID_ARG;
  *bytes = (uint64_t)mm::wide_sharded::kDoubles * sizeof(double);
  return MM_OK;
}

extern "C" int32_t mm_policy_wide_train_partial(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                                int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                                const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic,
                                                int32_t hidden, int32_t n_a, float clip_param, int32_t critic_loss,
                                                const float *adv_sums, const float *advantages, const int32_t *count, double *shard,
                                                float *logp_taken, float *value, float *ratio, void *scratch, uint64_t scratch_bytes,
                                                MMStream stream, int64_t chunk) {
  using namespace mm::wide_sharded;
  namespace wt = mm::wt;
  // everything that can refuse the call comes before the first enqueue
  if (!aligned(count, 4) || !aligned(shard, 16)) return MM_ERR_INVALID_ARG;
  float *sc = (float *)scratch;
  int *local = (int *)sc;  // prep's count: the rank's own
  wt::PassArgs p = {};     // the rank's samples
  p.obs = obs; p.obs_stride = obs_stride; p.n = n; p.n_s = n_s; p.actions = actions; p.act_stride = act_stride; p.returns = returns;
  p.ret_stride = ret_stride; p.old_logp = old_logp; p.valid = valid; p.n_a = n_a; p.clip_param = clip_param;
  p.huber = critic_loss == MM_PT_CRITIC_HUBER; p.adv_sums = adv_sums; p.advantages = advantages; p.count = count;  // (the WHOLE batch's B)
  const WideNet net[2] = {{actor, logp_taken, ratio}, {critic, value, nullptr}};
  ChunkLayout L;
  if (!wide_args_ok(p, net, hidden, critic_loss, chunk, scratch, scratch_bytes, L)) return MM_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const double config = config_word(n_s, n_a, actor && adv_sums, p.huber, (actor ? kNetActor : 0) | (critic ? kNetCritic : 0));
  if (hipMemsetAsync(shard, 0, kDoubles * sizeof(double), s) != hipSuccess) return MM_ERR_DEVICE;
  if (n == 0) {  // an empty shard: a valid all-zero block with local count 0
    hipLaunchKernelGGL(wide_shard_tail_kernel, dim3(1), dim3(256), 0, s, (const double *)nullptr, (const double *)nullptr, 0ll,
                       (const int *)count, (const int *)nullptr, config, (int)n_s, (int)n_a, shard);
    return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
  }
  const double *lossp = (const double *)(sc + L.lossp);  // the actor's, then the critic's
  if (hipMemsetAsync(local, 0, sizeof(int), s) != hipSuccess) return MM_ERR_DEVICE;
  wide_passes(s, p, net, chunk, L, sc, shard + kAcc);
  hipLaunchKernelGGL(wide_shard_tail_kernel, dim3(2 + (2 * Part::kSize + 255) / 256), dim3(256), 0, s, actor ? lossp : nullptr,
                     critic ? lossp + L.ntiles : nullptr, L.ntiles, (const int *)count, (const int *)local, config, (int)n_s,
                     (int)n_a, shard);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

extern "C" int32_t mm_policy_wide_train_finish(const double *blocks, int32_t n_blocks, int64_t block_stride, int32_t n_s, int32_t n_a,
                                               const MMMlpParams *actor_grads, const MMMlpParams *critic_grads, float *loss,
                                               MMStream stream) {
  using namespace mm::wide_sharded;
  if ((!actor_grads && !critic_grads) || !loss || !aligned(blocks, 8)) return MM_ERR_INVALID_ARG;
  if ((actor_grads && !complete(actor_grads)) || (critic_grads && !complete(critic_grads))) return MM_ERR_INVALID_ARG;
  if (n_blocks < 1 || n_blocks > 64 || block_stride < kDoubles || n_s < 25 || n_s > 32 || n_a < 1 || n_a > 8) return MM_ERR_INVALID_ARG;
  FinishArgs a = {};
  a.blocks = blocks; a.stride = block_stride; a.n_blocks = n_blocks; a.n_s = n_s; a.n_a = n_a; a.loss = loss;
  if (actor_grads) { a.want |= kNetActor; a.nelem_a = wide_elems(n_s, kWide, n_a); a.actor = *actor_grads; }
  if (critic_grads) { a.want |= kNetCritic; a.nelem_c = wide_elems(n_s, kWide + n_a, 1); a.critic = *critic_grads; }
  hipLaunchKernelGGL(wide_shard_finish_kernel, dim3((a.nelem_a + a.nelem_c + 255) / 256 + 1), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
