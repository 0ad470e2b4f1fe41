// mm_opt_step_bank.hip -- mm_opt_step's tail for K stacked members per prototype group in one launch (include/mm_opt_step.h:
// mm_opt_step_bank): clip_grad_norm_ + RMSprop / Adam + soft target update of n_groups * K networks, one workgroup each.
//
// Workgroup b serves member b % K of prototype group b / K.  It copies the prototype's table into LDS as opt_step_kernel does,
// then moves every tensor pointer by k * count elements, the step counter and the norm by k, and takes bit k of soft_mask as its
// blend flag; from there on the two phases are opt_step_kernel's, statement for statement, on the pieces of mm_opt_step_dev.h
// (the table, tensor_of, update, phase2).  The kernel body is written out here rather than shared: opt_step_kernel keeps its
// text and its recorded figures.  A member's 16-byte accesses need k * count to keep the prototype's alignment; where it does not
// the tensor takes the element path, which computes the same bits.
#include "mm_opt_step_dev.h"
#include "../../include/mm_policy_bank.h"  // MM_BANK_MAX_GROUPS

namespace mm {
namespace opt {

static_assert(sizeof(Args) + 16 <= 4096, "the table, K and the mask must fit the kernel arguments");

__global__ __launch_bounds__(kThreads) void opt_step_bank_kernel(const Args args, const int K, const unsigned long long soft_mask) {
  __shared__ Group G;
  __shared__ double wave_sum[kWaves];
  __shared__ Scalars sc;
  const int tid = threadIdx.x;
  const int gi = (int)blockIdx.x / K, member = (int)blockIdx.x - gi * K;
  {  // the prototype's table: kernel argument -> LDS, 4 bytes per thread
    const unsigned *src = (const unsigned *)&args.g[gi];
    unsigned *dst = (unsigned *)&G;
    for (int i = tid; i < (int)(sizeof(Group) / 4); i += kThreads) dst[i] = src[i];
  }
  __syncthreads();
  if (tid == 0) {  // the prototype -> this member
    unsigned vec = 0;
    for (int i = 0; i < G.n_tensors; i++) {
      const int chunks = G.chunk_start[i + 1] - G.chunk_start[i];
      if (chunks == 0) continue;
      const long long off = (long long)member * ((long long)(chunks - 1) * 4 + G.tail[i]);
      Tensor T = G.t[i];
      T.param += off;
      if (T.grad) T.grad += off;
      if (T.state1) T.state1 += off;
      if (T.state2) T.state2 += off;
      if (T.target) T.target += off;
      G.t[i] = T;
      if (((G.vec_mask >> i) & 1u) && (off & 3) == 0) vec |= 1u << i;
    }
    G.vec_mask = vec;
    if (G.step) G.step += member;
    if (G.grad_norm) G.grad_norm += member;
    G.blend = (int)((soft_mask >> member) & 1ull);
  }
  __syncthreads();
  if (G.n_tensors == 0) return;
  if (G.algo == MM_OPT_BLEND) {
    const Scalars none = {1.f, 0.f, 1.f};
    phase2<MM_OPT_BLEND>(G, none, tid);
    return;
  }
  // ---- phase 1: sum of squares in double, fixed order (opt_step_kernel's)
  double sum = 0.0;
  if (G.clip || G.grad_norm) {
    const int total = G.chunk_start[G.n_tensors];
    for (int c = tid; c < total; c += kThreads) {
      const int k = tensor_of(G.chunk_start, G.n_tensors, c);
      const gf *gp = (const gf *)G.t[k].grad + (long long)(c - G.chunk_start[k]) * 4;
      const int len = (c + 1 == G.chunk_start[k + 1]) ? G.tail[k] : 4;
      if (((G.vec_mask >> k) & 1u) && len == 4) {
        const v4f g = *(const gv4f *)gp;
        sum += (double)g.x * (double)g.x; sum += (double)g.y * (double)g.y;
        sum += (double)g.z * (double)g.z; sum += (double)g.w * (double)g.w;
      } else {
        for (int e = 0; e < len; e++) sum += (double)gp[e] * (double)gp[e];
      }
    }
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    Scalars s = {1.f, 0.f, 1.f};
    if (G.clip || G.grad_norm) {
      double all = 0.0;
      for (int w = 0; w < kWaves; w++) all += wave_sum[w];
      const float total = (float)sqrt(all);
      if (G.grad_norm) *(gf *)G.grad_norm = total;
      if (G.clip) {
        const float raw = (1.0f / (total + 1e-6f)) * G.max_norm;
        s.coef = raw > 1.0f ? 1.0f : raw;
      }
    }
    int step = 0;
    if (G.step) {
      __attribute__((address_space(1))) int *const sp = (__attribute__((address_space(1))) int *)G.step;
      *sp = step = *sp + 1;
    }
    if (G.algo == MM_OPT_ADAM) {
      const double bc1 = 1.0 - pow(G.beta1, (double)step), bc2 = 1.0 - pow(G.beta2, (double)step);
      s.neg_step_size = (float)(-(G.lr / bc1));
      s.bc2_sqrt = (float)sqrt(bc2);
    }
    sc = s;
  }
  __syncthreads();
  // ---- phase 2: the element update
  const Scalars s = sc;
  if (G.algo == MM_OPT_ADAM) phase2<MM_OPT_ADAM>(G, s, tid);
  else phase2<MM_OPT_RMSPROP>(G, s, tid);
}

}  // namespace opt
}  // namespace mm

extern "C" int32_t mm_opt_step_bank(const MMOptGroup *groups, int32_t n_groups, int32_t K, uint64_t soft_mask, MMStream stream) {
  using namespace mm::opt;
  if (!groups) return refuse("mm_opt_step_bank: groups is NULL");
  if (n_groups < 1 || n_groups > MM_OPT_MAX_GROUPS)
    return refuse("mm_opt_step_bank: n_groups %d is outside 1..%d", n_groups, MM_OPT_MAX_GROUPS);
  if (K < 1 || K > MM_BANK_MAX_GROUPS) return refuse("mm_opt_step_bank: K %d is outside 1..%d", K, MM_BANK_MAX_GROUPS);
  const uint64_t members = K == 64 ? ~0ull : ((1ull << K) - 1);
  Args args;
  bool work = false;
  for (int g = 0; g < n_groups; g++) {
    MMOptGroup proto = groups[g];
    proto.soft_update = (soft_mask & members) != 0;  // (a target is needed as soon as one member blends)
    const int rc = prepare(proto, g, args.g[g]);
    if (rc != MM_OK) return rc;
    work = work || args.g[g].n_tensors > 0;
  }
  if (!work) return MM_OK;
  hipLaunchKernelGGL(opt_step_bank_kernel, dim3(n_groups * K), dim3(kThreads), 0, (hipStream_t)stream, args, (int)K,
                     (unsigned long long)soft_mask);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    char text[240];
    snprintf(text, sizeof text, "mm_opt_step_bank: launch failed: %s", hipGetErrorString(e));
    mm_set_thread_error(text);
    return MM_ERR_DEVICE;
  }
  return MM_OK;
}
