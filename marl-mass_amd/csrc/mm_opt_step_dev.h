// mm_opt_step_dev.h -- what mm_opt_step.hip and mm_opt_step_bank.hip share: the kernel-side table of one group, the element
// update (phase 2) and the host-side check that turns an MMOptGroup into that table.  The kernels themselves stay in their files:
// opt_step_kernel keeps its text and its recorded figures (profiles/opt_step).
#ifndef MM_OPT_STEP_DEV_H
#define MM_OPT_STEP_DEV_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "mm_handle.h"
#include "../../include/mm_opt_step.h"

namespace mm {
namespace opt {

constexpr int kThreads = 1024, kWaves = kThreads / 64, kMaxT = MM_OPT_MAX_TENSORS;

// The tensors are device memory, but a pointer that has been through the LDS copy of the table is a generic one to the
// compiler (flat accesses, which also wait on the LDS counter): say that they are global.
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gf;
typedef __attribute__((address_space(1))) v4f gv4f;

struct Tensor {
  float *param;
  const float *grad;
  float *state1, *state2, *target;
};

// What a workgroup needs of one group: hyperparameters already narrowed where torch narrows them.
struct Group {
  Tensor t[kMaxT];
  int chunk_start[kMaxT + 1];  // chunk_start[n_tensors] = the group's chunk count; later entries repeat it
  unsigned char tail[kMaxT];   // elements of tensor k's last chunk, 1..4
  unsigned vec_mask;           // bit k: every pointer of tensor k that this call touches is 16-byte aligned
  int algo, n_tensors, blend, clip;
  int *step;
  float *grad_norm;
  double lr, beta1, beta2;               // Adam's bias corrections are taken in double
  float decay, one_minus_decay;          // RMSprop: alpha, 1 - alpha | Adam: beta2, 1 - beta2
  float lerp_w;                          // Adam: 1 - beta1
  float neg_lr, eps, max_norm, tau, one_minus_tau;
};

struct Args {
  Group g[MM_OPT_MAX_GROUPS];
};
static_assert(sizeof(Args) <= 4096, "the table must fit a kernel argument");

struct Scalars {  // what phase 2 needs from phase 1
  float coef, neg_step_size, bc2_sqrt;
};

__device__ __forceinline__ int tensor_of(const int *chunk_start, int n_tensors, int c) {
  int k = 0;
#pragma unroll
  for (int j = 1; j < kMaxT; j++) k += (j < n_tensors && c >= chunk_start[j]) ? 1 : 0;  // (empty tensors: equal starts, skipped)
  return k;
}

template <int ALGO>
__device__ __forceinline__ void update(const Group &G, const Scalars &s, float g, float &p, float &s1, float &s2) {
  g = g * s.coef;
  if (ALGO == MM_OPT_RMSPROP) {
    s1 = s1 * G.decay + (G.one_minus_decay * g) * g;
    p = p + G.neg_lr * (g / (sqrtf(s1) + G.eps));
  } else {
    const float w = G.lerp_w, d = g - s1;  // torch.lerp: the form is chosen by the weight
    s1 = fabsf(w) < 0.5f ? s1 + w * d : g - d * (1.0f - w);
    s2 = s2 * G.decay + (G.one_minus_decay * g) * g;
    p = p + s.neg_step_size * (s1 / (sqrtf(s2) / s.bc2_sqrt + G.eps));
  }
}

__device__ __forceinline__ float blend(const Group &G, float t, float p) { return G.one_minus_tau * t + G.tau * p; }

template <int ALGO>
__device__ __forceinline__ void phase2(const Group &G, const Scalars &s, int tid) {
  const int total = G.chunk_start[G.n_tensors];
  for (int c = tid; c < total; c += kThreads) {
    const int k = tensor_of(G.chunk_start, G.n_tensors, c);
    const Tensor T = G.t[k];
    const long long off = (long long)(c - G.chunk_start[k]) * 4;
    const int len = (c + 1 == G.chunk_start[k + 1]) ? G.tail[k] : 4;
    gf *const param = (gf *)T.param + off, *const state1 = (gf *)T.state1 + off, *const state2 = (gf *)T.state2 + off;
    gf *const target = (gf *)T.target + off;
    const gf *const grad = (const gf *)T.grad + off;
    if (((G.vec_mask >> k) & 1u) && len == 4) {
      v4f p = *(const gv4f *)param;
      if (ALGO != MM_OPT_BLEND) {
        const v4f g = *(const gv4f *)grad;
        v4f a = *(const gv4f *)state1, b = {0.f, 0.f, 0.f, 0.f};
        if (ALGO == MM_OPT_ADAM) b = *(const gv4f *)state2;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          float pe = p[e], ae = a[e], be = b[e];
          update<ALGO>(G, s, g[e], pe, ae, be);
          p[e] = pe; a[e] = ae; b[e] = be;
        }
        *(gv4f *)param = p;
        *(gv4f *)state1 = a;
        if (ALGO == MM_OPT_ADAM) *(gv4f *)state2 = b;
      }
      if (G.blend) {
        v4f t = *(const gv4f *)target;
        t.x = blend(G, t.x, p.x); t.y = blend(G, t.y, p.y); t.z = blend(G, t.z, p.z); t.w = blend(G, t.w, p.w);
        *(gv4f *)target = t;
      }
    } else {
      for (int e = 0; e < len; e++) {
        float p = param[e];
        if (ALGO != MM_OPT_BLEND) {
          float a = state1[e], b = 0.f;
          if (ALGO == MM_OPT_ADAM) b = state2[e];
          update<ALGO>(G, s, grad[e], p, a, b);
          param[e] = p;
          state1[e] = a;
          if (ALGO == MM_OPT_ADAM) state2[e] = b;
        }
        if (G.blend) target[e] = blend(G, target[e], p);
      }
    }
  }
}

static int refuse(const char *fmt, ...) {
  char text[240];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(text, sizeof text, fmt, ap);
  va_end(ap);
  mm_set_thread_error(text);
  return MM_ERR_INVALID_ARG;
}

static bool unit_interval_open(double x) { return x >= 0.0 && x < 1.0; }

// One host group -> the kernel's table; MM_OK or the refusal.
static int prepare(const MMOptGroup &in, int gi, Group &out) {
  out = Group{};
  const int algo = in.algo;
  if (algo != MM_OPT_RMSPROP && algo != MM_OPT_ADAM && algo != MM_OPT_BLEND)
    return refuse("mm_opt_step: group %d: unknown algo %d (MM_OPT_RMSPROP, MM_OPT_ADAM or MM_OPT_BLEND)", gi, algo);
  if (in.n_tensors < 0 || in.n_tensors > kMaxT)
    return refuse("mm_opt_step: group %d: n_tensors %d is outside 0..%d", gi, in.n_tensors, kMaxT);
  const bool optimise = algo != MM_OPT_BLEND, adam = algo == MM_OPT_ADAM;
  const bool blend = !optimise || in.soft_update != 0;
  if (optimise) {
    if (!(in.lr >= 0.0) || !isfinite(in.lr)) return refuse("mm_opt_step: group %d: lr must be finite and >= 0", gi);
    if (!(in.eps > 0.0)) return refuse("mm_opt_step: group %d: eps must be > 0", gi);
    if (!unit_interval_open(in.alpha_or_beta1))
      return refuse("mm_opt_step: group %d: %s must be in [0, 1)", gi, adam ? "beta1" : "alpha");
    if (adam && !unit_interval_open(in.beta2)) return refuse("mm_opt_step: group %d: beta2 must be in [0, 1)", gi);
    if (in.max_grad_norm != in.max_grad_norm) return refuse("mm_opt_step: group %d: max_grad_norm is NaN", gi);
    if (adam && !in.step && in.n_tensors > 0) return refuse("mm_opt_step: group %d: Adam needs the device step counter", gi);
    if (((uintptr_t)in.step & 3u) || ((uintptr_t)in.grad_norm & 3u))
      return refuse("mm_opt_step: group %d: step / grad_norm must be 4-byte aligned", gi);
  }
  if (blend && !(in.tau >= 0.0 && in.tau <= 1.0)) return refuse("mm_opt_step: group %d: tau must be in [0, 1]", gi);
  long long chunks = 0;
  for (int k = 0; k < in.n_tensors; k++) {
    const long long cnt = in.count[k];
    if (cnt < 0) return refuse("mm_opt_step: group %d: tensor %d has a negative count", gi, k);
    out.chunk_start[k] = (int)chunks;
    if (cnt == 0) continue;
    const void *used[5] = {in.param[k], optimise ? in.grad[k] : nullptr, optimise ? in.state1[k] : nullptr,
                           adam ? in.state2[k] : nullptr, blend ? in.target[k] : nullptr};
    static const char *const what[5] = {"param", "grad", "state1", "state2 (Adam's exp_avg_sq)", "target"};
    const bool need[5] = {true, optimise, optimise, adam, blend};
    uintptr_t bits = 0;
    for (int j = 0; j < 5; j++) {
      if (!need[j]) continue;
      if (!used[j]) return refuse("mm_opt_step: group %d: tensor %d has no %s", gi, k, what[j]);
      bits |= (uintptr_t)used[j];
    }
    if (bits & 3u) return refuse("mm_opt_step: group %d: tensor %d has a pointer that is not 4-byte aligned", gi, k);
    if (!(bits & 15u)) out.vec_mask |= 1u << k;
    out.t[k] = Tensor{in.param[k], in.grad[k], in.state1[k], in.state2[k], in.target[k]};
    out.tail[k] = (unsigned char)(((cnt - 1) & 3) + 1);
    chunks += (cnt + 3) / 4;
    if (chunks > 0x7FFFFFFFll) return refuse("mm_opt_step: group %d holds more than 2^33 elements", gi);
  }
  for (int k = in.n_tensors; k <= kMaxT; k++) out.chunk_start[k] = (int)chunks;
  out.algo = algo;
  out.n_tensors = chunks ? in.n_tensors : 0;  // (nothing but empty tensors: nothing to do)
  out.blend = blend;
  out.clip = optimise && in.max_grad_norm >= 0.0;
  out.step = optimise ? in.step : nullptr;
  out.grad_norm = optimise ? in.grad_norm : nullptr;
  out.lr = in.lr; out.beta1 = in.alpha_or_beta1; out.beta2 = in.beta2;
  const double decay = adam ? in.beta2 : in.alpha_or_beta1;
  out.decay = (float)decay;
  out.one_minus_decay = (float)(1.0 - decay);
  out.lerp_w = (float)(1.0 - in.alpha_or_beta1);
  out.neg_lr = (float)(-in.lr);
  out.eps = (float)in.eps;
  out.max_norm = (float)in.max_grad_norm;
  out.tau = (float)in.tau;
  out.one_minus_tau = (float)(1.0 - in.tau);
  return MM_OK;
}

}  // namespace opt
}  // namespace mm
#endif
