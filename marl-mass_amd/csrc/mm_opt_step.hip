// mm_opt_step.hip -- clip_grad_norm_ + RMSprop / Adam + soft target update of up to four networks in one launch
// (include/mm_opt_step.h: the semantics, which are torch's float32 arithmetic).
//
// One workgroup of 1024 threads per group.  A group's tensors are seen as ONE list of 4-element chunks (chunk_start[k] = the
// first chunk of tensor k, computed on the host), so a thread's share -- chunks tid, tid + 1024, ... -- is a handful of
// independent 16-byte accesses whatever the tensor sizes are, instead of one dependent loop per tensor (twelve tensors of
// 1 .. 20 480 elements in the shared actor-critic).  A chunk is accessed as one float4 where every pointer of its tensor is
// 16-byte aligned and the chunk is whole, element by element otherwise (unaligned tensors, the last chunk of a tensor).
// The pointer table is a by-value kernel argument; each workgroup copies its group's table into LDS, because the tensor of a
// chunk differs from lane to lane.
//
// Phase 1 (RMSprop / Adam groups): the sum of squares of the gradients, one double per thread, reduced inside the wave by
// __shfl_xor and across the 16 waves through LDS in a fixed order; thread 0 turns it into the clipping coefficient, increments
// the device step counter and, for Adam, takes the two bias corrections in double.  Phase 2, after the barrier: the
// element update.  The order of every sum is fixed: two calls on equal inputs are bit-identical.
#include "mm_opt_step_dev.h"

namespace mm {
namespace opt {

__global__ __launch_bounds__(kThreads) void opt_step_kernel(const Args args) {
  __shared__ Group G;
  __shared__ double wave_sum[kWaves];
  __shared__ Scalars sc;
  const int tid = threadIdx.x;
  {  // this group's table: kernel argument -> LDS, 4 bytes per thread
    const unsigned *src = (const unsigned *)&args.g[blockIdx.x];
    unsigned *dst = (unsigned *)&G;
    for (int i = tid; i < (int)(sizeof(Group) / 4); i += kThreads) dst[i] = src[i];
  }
  __syncthreads();
  if (G.n_tensors == 0) return;
  if (G.algo == MM_OPT_BLEND) {
    const Scalars none = {1.f, 0.f, 1.f};
    phase2<MM_OPT_BLEND>(G, none, tid);
    return;
  }
  // ---- phase 1: sum of squares in double, fixed order ------------------------------------------------------------------
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
      // torch: clip_coef = max_norm / (total_norm + 1e-6), which a Python float over a tensor evaluates as reciprocal * max_norm
      if (G.clip) {
        const float raw = (1.0f / (total + 1e-6f)) * G.max_norm;
        s.coef = raw > 1.0f ? 1.0f : raw;  // torch.clamp(max = 1): a NaN stays a NaN
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
  // ---- phase 2: the element update ----------------------------------------------------------------------------------------
  const Scalars s = sc;
  if (G.algo == MM_OPT_ADAM) phase2<MM_OPT_ADAM>(G, s, tid);
  else phase2<MM_OPT_RMSPROP>(G, s, tid);
}

}  // namespace opt
}  // namespace mm

extern "C" int32_t mm_opt_step(const MMOptGroup *groups, int32_t n_groups, MMStream stream) {
  using namespace mm::opt;
  if (!groups) return refuse("mm_opt_step: groups is NULL");
  if (n_groups < 1 || n_groups > MM_OPT_MAX_GROUPS) return refuse("mm_opt_step: n_groups %d is outside 1..%d", n_groups, MM_OPT_MAX_GROUPS);
  Args args;
  bool work = false;
  for (int g = 0; g < n_groups; g++) {
    const int rc = prepare(groups[g], g, args.g[g]);
    if (rc != MM_OK) return rc;
    work = work || args.g[g].n_tensors > 0;
  }
  if (!work) return MM_OK;
  hipLaunchKernelGGL(opt_step_kernel, dim3(n_groups), dim3(kThreads), 0, (hipStream_t)stream, args);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    char text[240];
    snprintf(text, sizeof text, "mm_opt_step: launch failed: %s", hipGetErrorString(e));
    mm_set_thread_error(text);
    return MM_ERR_DEVICE;
  }
  return MM_OK;
}
