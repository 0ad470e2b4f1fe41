// mm_main.hip -- the C ABI of include/mm_abi.h and the main object of the step library (mm_step_host.h lists the ten): handle
// and configuration, reset / observe, the mm_step dispatch with the CAV-only exact-mode step kernels, the stand-alone shield and
// QP entries, the metrics flush, and the kernels that are no templates (math / geometry probes, categorical sampler, returns,
// the f32-MFMA policy kernel of the rollout counterpart).
#include "mm_step_host.h"

// stand-alone batched shield QP (cbf.py:110-161), one thread (lane) per QP: the exact KKT point, or (solver ==
// MM_QP_IPM) the iterate of cvxopt's interior-point algorithm with its status and iteration count (include/mm_qp.h)
__global__ void qp_kernel(int n, const double *__restrict__ G, const double *__restrict__ h,
                          const int32_t *__restrict__ rows, int solver, double *__restrict__ u, uint8_t *status,
                          int32_t *iters, int *err) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const double *g = G + (long long)k * 12, *hh = h + (long long)k * 4;
  const int m = rows[k];
  // only the G of get_G (cbf.py:288-304,386-403): [a 0 -1; 1 0 0; -1 0 0] (+ [a 0 -1])
  bool ok = (m == 3 || m == 4) && g[1] == 0.0 && g[2] == -1.0 && g[3] == 1.0 && g[4] == 0.0 && g[5] == 0.0 && g[6] == -1.0 &&
            g[7] == 0.0 && g[8] == 0.0;
  if (ok && m == 4) ok = g[9] == g[0] && g[10] == 0.0 && g[11] == -1.0;
  if (iters) iters[k] = 0;
  if (!ok) {
    u[k * 3 + 0] = u[k * 3 + 1] = u[k * 3 + 2] = __builtin_nan("");
    if (status) status[k] = MM_QPS_BAD_STRUCTURE;
    atomicOr(err, MM_LATCH_BAD_QP);
    return;
  }
  const double a = g[0];
  if (solver == MM_QP_IPM) {
    double d, sl;
    int it;
    const int opt = mm_qp_ipm_cbf(a, hh[0], hh[1], hh[2], m == 4 ? hh[3] : 0.0, m, &d, &sl, &it);
    u[k * 3 + 0] = d; u[k * 3 + 1] = 0.0; u[k * 3 + 2] = sl;
    if (status) status[k] = opt ? MM_QPS_OPTIMAL : MM_QPS_UNKNOWN;
    if (iters) iters[k] = it;
    return;
  }
  double hc = hh[0];
  if (m == 4 && hh[3] < hc) hc = hh[3];
  double d;
  if (a > 0) d = fmin(0.0, hc / a);
  else if (a < 0) d = fmax(0.0, hc / a);
  else d = 0.0;
  d = fmin(fmax(d, -hh[2]), hh[1]);
  const double s = a * d - hc;
  u[k * 3 + 0] = d; u[k * 3 + 1] = 0.0; u[k * 3 + 2] = s > 0 ? s : 0.0;
  if (status) status[k] = MM_QPS_OPTIMAL;
}

// folds the per-wave metric partials of one step launch into the caller's accumulator (7 sums + 1 min): each block takes
// 256 waves' partials (8 independent loads per thread in flight), reduces them in LDS and issues 8 atomics
constexpr int kFlushWaves = 256;
// reset: the partials were accumulated over several launches (mm_defer_metrics) -- put every row back to the identity
__global__ __launch_bounds__(256) void metrics_flush_kernel(double *partial, long long waves, double *metrics, int reset) {
  __shared__ double s_p[32][8];
  const int k = threadIdx.x & 7, r = threadIdx.x >> 3;
  const long long w0 = (long long)blockIdx.x * kFlushWaves;
  double x[kFlushWaves / 32];
#pragma unroll
  for (int j = 0; j < kFlushWaves / 32; j++) {
    const long long w = w0 + r + 32 * j;
    x[j] = w < waves ? partial[w * 8 + k] : (k == 7 ? INFINITY : 0.0);
    if (reset && w < waves) partial[w * 8 + k] = k == 7 ? INFINITY : 0.0;
  }
  double acc = k == 7 ? INFINITY : 0.0;
#pragma unroll
  for (int j = 0; j < kFlushWaves / 32; j++) acc = k == 7 ? fmin(acc, x[j]) : acc + x[j];
  if (reset == 2) return;  // (mm_defer_metrics: rows to the identity, nothing folded -- block-uniform)
  s_p[r][k] = acc;
  __syncthreads();
  if (threadIdx.x < 8) {
    double t = k == 7 ? INFINITY : 0.0;
    for (int j = 0; j < 32; j++) t = k == 7 ? fmin(t, s_p[j][k]) : t + s_p[j][k];
    if (k == 7) atomic_min_d(&metrics[7], t);
    else atomicAdd(&metrics[k], t);
  }
}

// ------------------------------------------------------------------------------------------------
// host side: C ABI
// ------------------------------------------------------------------------------------------------
static uint64_t align256(uint64_t x) { return (x + 255u) & ~(uint64_t)255u; }

extern "C" int32_t mm_abi_version(void) { return MM_ABI_VERSION; }

const MMHandleHead *mm_handle_head(MMHandle h) { return h; }

extern "C" int32_t mm_state_layout(int32_t E, int32_t N, MMStateLayout *out) {
  if (!out || E <= 0 || N <= 0 || N > MM_MAX_AGENTS) return MM_ERR_INVALID_ARG;
  uint64_t A = (uint64_t)E * (uint64_t)N, off = 0;
  out->f64_offset = off; off = align256(off + A * 8u * MM_F_COUNT);
  out->u8_offset = off; off = align256(off + A * MM_B_COUNT);
  out->env_offset = off; off = align256(off + (uint64_t)E * 4u * MM_E_COUNT);
  out->seed_offset = off; off = align256(off + (uint64_t)E * 8u);
  out->total_bytes = off;
  return MM_OK;
}

static int check_cfg(const MMConfig *c, int N, char *err) {
  if (!c || c->abi_version != MM_ABI_VERSION) { snprintf(err, 256, "ABI version mismatch"); return MM_ERR_INVALID_ARG; }
  if (c->env_kind != MM_ENV_V0 && c->env_kind != MM_ENV_V1 && c->env_kind != MM_ENV_HDV_V1) { snprintf(err, 256, "unknown env_kind %d", c->env_kind); return MM_ERR_INVALID_ARG; }
  if (c->env_kind == MM_ENV_HDV_V1) {  // MergeEnvLCHDV: no controlled vehicle, so nothing a shield or a CAV setting could act on
    if (c->shield != MM_SHIELD_NONE) { snprintf(err, 256, "merge-multi-agent-hdv-v1 has no controlled vehicle: shield must be none, got %d", c->shield); return MM_ERR_INVALID_ARG; }
    if (c->lateral_control != MM_LATERAL_STEER) { snprintf(err, 256, "merge-multi-agent-hdv-v1 has no controlled vehicle: lateral_control must be steer"); return MM_ERR_INVALID_ARG; }
    if (c->n_hdv != 0) { snprintf(err, 256, "merge-multi-agent-hdv-v1: every vehicle is an HDV, n_hdv must be 0 (got %d)", c->n_hdv); return MM_ERR_INVALID_ARG; }
  }
  if (c->shield < MM_SHIELD_NONE || c->shield > MM_SHIELD_MASS) { snprintf(err, 256, "Undefined safety_type:%d", c->shield); return MM_ERR_INVALID_ARG; }
  if (c->policy_frequency <= 0 || c->simulation_frequency < c->policy_frequency ||
      c->simulation_frequency / c->policy_frequency > 3) { snprintf(err, 256, "unsupported frequencies"); return MM_ERR_INVALID_ARG; }
  if (N > 12) { snprintf(err, 256, "N=%d exceeds the 6+6 spawn slots", N); return MM_ERR_INVALID_ARG; }
  if (c->env_kind != MM_ENV_HDV_V1 && (c->n_hdv < 0 || c->n_hdv >= N)) { snprintf(err, 256, "n_hdv=%d must leave at least one controlled vehicle of N=%d", c->n_hdv, N); return MM_ERR_INVALID_ARG; }
  if (c->qp_solver != MM_QP_EXACT && c->qp_solver != MM_QP_IPM) { snprintf(err, 256, "unknown qp_solver %d", c->qp_solver); return MM_ERR_INVALID_ARG; }
  // every vehicle composition this configuration can produce -- fixed counts, or any per-episode draw incl. the
  // reset(num_CAV=k) override -- must fit the N slots and the six spawn points per road (the reference raises from
  // np.random.choice(replace=False), merge_env_v1.py:284-320); checked here so that mm_create / mm_set_config refuse it
  // before any (auto-)reset can meet it
  if (mm_counts_check(c, N, 0, err, 256)) return MM_ERR_INVALID_ARG;
  return MM_OK;
}

// device memory of the hand-off planes (idempotent; the caller holds a DeviceGuard)
static hipError_t ensure_sweep(MMHandle_ *h) {
  if (h->sweep_mem || !steps_split(h)) return hipSuccess;
  const uint64_t Ep = ((uint64_t)h->E + 63u) & ~(uint64_t)63u, N = (uint64_t)h->N;
  const uint64_t bF = align256(Ep * N * 8u * SW_F_COUNT), bI = align256(Ep * N * 4u * SW_I_COUNT), bO = align256(Ep * N), bE = 2 * align256(Ep);
  unsigned char *m = nullptr;
  hipError_t rc = hipMalloc((void **)&m, bF + bI + bO + bE);
  if (rc != hipSuccess) return rc;
  rc = hipMemset(m, 0, bF + bI + bO + bE);
  if (rc != hipSuccess) { (void)hipFree(m); return rc; }
  h->sweep_mem = m;
  h->sweep.F = (double *)m; h->sweep.I = (int *)(m + bF); h->sweep.order = m + bF + bI; h->sweep.envf = m + bF + bI + bO;
  h->sweep.urgent = h->sweep.envf + align256(Ep);
  h->sweep.Ep = (long long)Ep; h->sweep.N = h->N;
  return hipSuccess;
}

// device memory of the carried pose planes (idempotent; the caller holds a DeviceGuard).  Zeroed: no key of a zeroed plane
// carries the "written" mark, so a fresh handle derives everything in its first step.
static bool carries_pose(const MMHandle_ *h) { return h->cfg.env_kind == MM_ENV_V1 && h->cfg.shield != MM_SHIELD_NONE; }
static hipError_t ensure_pose(MMHandle_ *h) {
  if (h->pose_mem || !carries_pose(h)) return hipSuccess;
  const uint64_t A = (uint64_t)h->E * (uint64_t)h->N;
  const uint64_t bF = align256(A * 8u * PB_F_COUNT), bI = align256(A * 4u);
  unsigned char *m = nullptr;
  hipError_t rc = hipMalloc((void **)&m, bF + bI);
  if (rc != hipSuccess) return rc;
  rc = hipMemset(m, 0, bF + bI);
  if (rc != hipSuccess) { (void)hipFree(m); return rc; }
  h->pose_mem = m;
  h->pose.F = (double *)m; h->pose.code = (int *)(m + bF);
  return hipSuccess;
}

static thread_local char g_create_err[256] = "null handle";  // why the last mm_create of this thread refused (there is no handle to ask)
void mm_set_thread_error(const char *text) { snprintf(g_create_err, sizeof g_create_err, "%s", text); }  // (mm_handle.h)
// The host-side entries that touch the runtime outside a stream (allocation, latch poll, drain) must address the handle's
// device, but the caller's current device is the caller's: it is put back on exit (a two-GPU process polling the env of the
// other GPU would otherwise find torch's current device changed under it).
struct DeviceGuard {
  int prev = -1;
  hipError_t rc;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    rc = hipSetDevice(device);
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
static int hip_fail(MMHandle h, hipError_t e, const char *what) {
  snprintf(h->err, sizeof h->err, "%s: %s", what, hipGetErrorString(e));
  return MM_ERR_DEVICE;
}

extern "C" int32_t mm_create(const MMConfig *cfg, int32_t E, int32_t N, int32_t device, void *state,
                             uint64_t state_bytes, int64_t first_env, MMHandle *out) {
  if (!out || !state) return MM_ERR_INVALID_ARG;
  MMHandle h = (MMHandle)calloc(1, sizeof(struct MMHandle_));
  snprintf(h->err, sizeof h->err, "mm_create: E, N, the state buffer (size, 256-byte alignment) or the configuration is invalid");
  if (mm_state_layout(E, N, &h->lay) != MM_OK || state_bytes < h->lay.total_bytes ||
      ((uintptr_t)state & 255u) || check_cfg(cfg, N, h->err) != MM_OK) {
    snprintf(g_create_err, sizeof g_create_err, "%s", h->err);
    free(h);
    return MM_ERR_INVALID_ARG;
  }
  h->err[0] = 0;
  h->cfg = *cfg; h->E = E; h->N = N; h->device = device; h->state = (unsigned char *)state;
  h->first_env = first_env;
  // per-env seed plane: cfg.seed + global env index
  uint64_t *tmp = (uint64_t *)malloc((size_t)E * 8u);
  for (int64_t e = 0; e < E; e++) tmp[e] = cfg->seed + (uint64_t)(first_env + e);
  DeviceGuard dg(device);
  hipError_t rc = dg.rc;
  if (rc == hipSuccess) {
    int cus = 0;
    rc = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    h->n_simd = 4 * cus;
  }
  if (rc == hipSuccess) rc = hipMemcpy(h->state + h->lay.seed_offset, tmp, (size_t)E * 8u, hipMemcpyHostToDevice);
  free(tmp);
  if (rc == hipSuccess) rc = hipMalloc((void **)&h->dev_err, MM_LW_COUNT * sizeof(int));
  if (rc == hipSuccess) rc = hipMemset(h->dev_err, 0, MM_LW_COUNT * sizeof(int));
  if (rc == hipSuccess) rc = ensure_sweep(h);
  if (rc == hipSuccess) rc = ensure_pose(h);
  if (rc != hipSuccess) {
    if (h->dev_err) (void)hipFree(h->dev_err);
    if (h->sweep_mem) (void)hipFree(h->sweep_mem);
    free(h);
    return MM_ERR_DEVICE;
  }
  *out = h;
  return MM_OK;
}
extern "C" int32_t mm_destroy(MMHandle h) {
  if (!h) return MM_OK;
  // launches of this handle may still be in flight and they write its error latch: drain the device first
  DeviceGuard dg(h->device);
  hipError_t rc = dg.rc;
  if (rc == hipSuccess) rc = hipDeviceSynchronize();
  if (h->dev_err) (void)hipFree(h->dev_err);
  if (h->metrics_partial) (void)hipFree(h->metrics_partial);
  if (h->sweep_mem) (void)hipFree(h->sweep_mem);
  if (h->pose_mem) (void)hipFree(h->pose_mem);
  free(h);
  return rc == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
// include/mm_abi.h: conditions the reference raises inside step(), latched by the kernels
static int poll_latch(MMHandle h, int word, MMStream stream) {
  int bits = 0;
  DeviceGuard dg(h->device);  // (a multi-GPU process may have another device current)
  hipError_t rc = dg.rc;
  if (rc == hipSuccess) rc = hipStreamSynchronize((hipStream_t)stream);
  if (rc == hipSuccess) rc = hipMemcpy(&bits, h->dev_err + word, sizeof bits, hipMemcpyDeviceToHost);
  if (rc == hipSuccess && bits) rc = hipMemset(h->dev_err + word, 0, sizeof(int));
  if (rc != hipSuccess) return hip_fail(h, rc, "error poll");
  if (!bits) return MM_OK;
  // every latched condition goes into the message; the return code is the most specific one
  snprintf(h->err, sizeof h->err, "%s%s%s%s",
           (bits & MM_LATCH_QP_BOUNDS) ? "Error in QP. Invalid accceleration; " : "",
           (bits & MM_LATCH_BAD_ACTION) ? "an action is outside 0..4; " : "",
           (bits & MM_LATCH_BAD_QP) ? "mm_shield_qp: G is not of the form get_G builds (cbf.py:288-304,386-403); " : "",
           (bits & MM_LATCH_INTERNAL) ? "internal: a kernel loop guard fired; " : "");
  if (bits & MM_LATCH_INTERNAL) return MM_ERR_DEVICE;
  if (bits & MM_LATCH_QP_BOUNDS) return MM_ERR_QP_BOUNDS;
  return MM_ERR_INVALID_ARG;
}
static void launch_metrics_flush(MMHandle h, hipStream_t s, int reset) {
  // per-step fold: the rows the launch just wrote; deferred fold: the whole buffer (rows nothing added to hold the identity)
  const long long waves = reset ? step_launch_waves(h) : step_launch_waves_now(h);
  hipLaunchKernelGGL(metrics_flush_kernel, dim3((unsigned)((waves + kFlushWaves - 1) / kFlushWaves)), dim3(256), 0, s,
                     h->metrics_partial, waves, h->metrics, reset);
}
extern "C" int32_t mm_flush_metrics(MMHandle h, MMStream stream) {
  if (!h) return MM_ERR_INVALID_ARG;
  if (!h->metrics_deferred || !h->metrics) return MM_OK;  // (not deferred: the caller's buffer is current after every step)
  DeviceGuard dg(h->device);  // (a multi-GPU process may have another device current: the launch belongs to the handle's)
  if (dg.rc != hipSuccess) return hip_fail(h, dg.rc, "metrics flush");
  launch_metrics_flush(h, (hipStream_t)stream, 1);
  const hipError_t rc = hipGetLastError();
  return rc == hipSuccess ? MM_OK : hip_fail(h, rc, "metrics flush");
}
extern "C" int32_t mm_defer_metrics(MMHandle h, int32_t deferred, MMStream stream) {
  if (!h) return MM_ERR_INVALID_ARG;
  if (deferred && !h->metrics) {
    snprintf(h->err, sizeof h->err, "mm_defer_metrics: no metrics buffer (mm_set_metrics_buffer first)");
    return MM_ERR_INVALID_ARG;
  }
  if ((deferred != 0) == (h->metrics_deferred != 0)) return MM_OK;
  DeviceGuard dg(h->device);
  if (dg.rc != hipSuccess) return hip_fail(h, dg.rc, "mm_defer_metrics");
  if (deferred) {  // every row to the identity (reset = 2: nothing is folded), then the step launches accumulate
    const long long waves = step_launch_waves(h);
    hipLaunchKernelGGL(metrics_flush_kernel, dim3((unsigned)((waves + kFlushWaves - 1) / kFlushWaves)), dim3(256), 0,
                       (hipStream_t)stream, h->metrics_partial, waves, (double *)nullptr, 2);
    h->metrics_deferred = 1;
  } else {
    launch_metrics_flush(h, (hipStream_t)stream, 1);
    h->metrics_deferred = 0;
  }
  const hipError_t rc = hipGetLastError();
  return rc == hipSuccess ? MM_OK : hip_fail(h, rc, "mm_defer_metrics");
}
extern "C" int32_t mm_poll_errors(MMHandle h, MMStream stream) {
  if (!h) return MM_ERR_INVALID_ARG;
  const int frc = mm_flush_metrics(h, stream);  // deferred metrics: a poll is where a rollout loop synchronises anyway
  if (frc != MM_OK) return frc;
  return poll_latch(h, MM_LW_STEP, stream);
}
extern "C" int32_t mm_set_config(MMHandle h, const MMConfig *cfg) {
  if (!h) return MM_ERR_INVALID_ARG;
  int rc = check_cfg(cfg, h->N, h->err);
  if (rc != MM_OK) return rc;
  if (h->envp && !envp_scope(cfg)) {
    snprintf(h->err, sizeof h->err, "mm_set_config: per-env parameters are set (mm_set_env_params) and exist for merge-multi-agent-v1 with the "
             "HSS or MASS shield only (env_kind %d, shield %d); clear them first", cfg->env_kind, cfg->shield);
    return MM_ERR_INVALID_ARG;
  }
  h->cfg = *cfg;
  DeviceGuard dg(h->device);  // (the new configuration may step in the split form: its hand-off planes are allocated here)
  hipError_t hrc = dg.rc;
  if (hrc == hipSuccess) hrc = ensure_sweep(h);
  if (hrc != hipSuccess) return hip_fail(h, hrc, "hand-off planes of the split interior-point step");
  hrc = ensure_pose(h);
  return hrc == hipSuccess ? MM_OK : hip_fail(h, hrc, "carried pose planes");
}
extern "C" int32_t mm_set_env_params(MMHandle h, const double *params) {  // include/mm_env_params.h
  if (!h) return MM_ERR_INVALID_ARG;
  if (params && !envp_scope(&h->cfg)) {
    snprintf(h->err, sizeof h->err, "mm_set_env_params: per-env cbf_eta / cbf_tau / HEADWAY_TIME exist for merge-multi-agent-v1 with the "
             "HSS or MASS shield only (env_kind %d, shield %d)", h->cfg.env_kind, h->cfg.shield);
    return MM_ERR_INVALID_ARG;
  }
  h->envp = params;
  if (params) return MM_OK;
  DeviceGuard dg(h->device);  // (off: the configuration may step in the split form again, whose planes are allocated outside mm_step)
  hipError_t hrc = dg.rc;
  if (hrc == hipSuccess) hrc = ensure_sweep(h);
  return hrc == hipSuccess ? MM_OK : hip_fail(h, hrc, "hand-off planes of the split interior-point step");
}
extern "C" int32_t mm_set_metrics_buffer(MMHandle h, double *metrics) {
  if (!h) return MM_ERR_INVALID_ARG;
  if (metrics && !h->metrics_partial) {  // per-wave partials of one step launch (allocated here, never inside step)
    const long long waves = step_launch_waves(h);
    DeviceGuard dg(h->device);
    hipError_t rc = dg.rc;
    if (rc == hipSuccess) rc = hipMalloc((void **)&h->metrics_partial, (size_t)waves * 8 * sizeof(double));
    if (rc != hipSuccess) return hip_fail(h, rc, "metrics partial buffer");
  }
  if (h->metrics_deferred && h->metrics && metrics != h->metrics) {
    // the partials were collected for the buffer that is being replaced: fold them into THAT one before the switch (there is
    // no stream argument here: the null stream, synchronised)
    DeviceGuard dg(h->device);
    hipError_t rc = dg.rc;
    if (rc == hipSuccess) { launch_metrics_flush(h, (hipStream_t)0, 1); rc = hipGetLastError(); }
    if (rc == hipSuccess) rc = hipStreamSynchronize((hipStream_t)0);
    if (rc != hipSuccess) return hip_fail(h, rc, "metrics flush before the buffer switch");
  }
  h->metrics = metrics;
  if (!metrics) h->metrics_deferred = 0;  // (no buffer, nothing to defer; what the partials held is dropped)
  return MM_OK;
}
extern "C" const char *mm_last_error(MMHandle h) { return h ? h->err : g_create_err; }

template <int G>
static void launch_reset_g(MMHandle h, int mode, const uint8_t *mask, const uint64_t *seeds, void *obs,
                           uint8_t *avail, hipStream_t s) {
  if (h->cfg.env_kind == MM_ENV_V1) launch_reset_t<G, MM_ENV_V1>(h, mode, mask, seeds, obs, avail, s);
  else launch_reset_t<G, MM_ENV_V0>(h, mode, mask, seeds, obs, avail, s);
}
static int launch_reset(MMHandle h, int mode, const uint8_t *mask, const uint64_t *seeds, void *obs,
                        uint8_t *avail, MMStream stream) {
  hipStream_t s = (hipStream_t)stream;
  if (h->cfg.env_kind == MM_ENV_HDV_V1) mm_launch_reset_idm(h, mode, mask, seeds, obs, avail, s);
  else {
#define MM_RESET_CASE(GG) launch_reset_g<GG>(h, mode, mask, seeds, obs, avail, s)
    MM_FOR_GROUP(group_size(h->N), MM_RESET_CASE, MM_NO_GROUP);
#undef MM_RESET_CASE
  }
  hipError_t rc = hipGetLastError();
  return rc == hipSuccess ? MM_OK : hip_fail(h, rc, "reset launch");
}

extern "C" int32_t mm_reset(MMHandle h, const uint8_t *env_mask, const uint64_t *seeds, void *obs,
                            uint8_t *avail, MMStream stream) {
  if (!h) return MM_ERR_INVALID_ARG;
  if (mm_counts_check(&h->cfg, h->N, 1, h->err, sizeof h->err)) return MM_ERR_INVALID_ARG;  // the device spawns N - n_hdv CAVs + n_hdv HDVs
  return launch_reset(h, 0, env_mask, seeds, obs, avail, stream);
}
extern "C" int32_t mm_init_from_kinematics(MMHandle h, const uint8_t *env_mask, MMStream stream) {
  if (!h) return MM_ERR_INVALID_ARG;
  return launch_reset(h, 1, env_mask, nullptr, nullptr, nullptr, stream);
}
extern "C" int32_t mm_observe(MMHandle h, void *obs, uint8_t *avail, MMStream stream) {
  if (!h) return MM_ERR_INVALID_ARG;
  return launch_reset(h, 2, nullptr, nullptr, obs, avail, stream);
}

// mixed traffic (cfg.n_hdv > 0) and steer_vel run the "general" kernels that carry the IDM/MOBIL code; the MM_QP_IPM
// fidelity mode has its own (general, literal-sweep) kernels; CAV-only batches keep the leaner instantiation of this object.
template <int G>
static void launch_step_g(MMHandle h, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
  if (fused_ipm(h)) mm_launch_step_ipm(h, actions, out, s);                // (mm_ipm.hip)
  else if (needs_general(h)) mm_launch_step_general(h, actions, out, s);  // (mm_general.hip)
  else launch_step_m<G, false>(h, actions, out, s);
}

extern "C" int32_t mm_step(MMHandle h, const int32_t *actions, const MMStepOut *out, MMStream stream) {
  if (!h || !out || (!actions && h->cfg.env_kind != MM_ENV_HDV_V1)) return MM_ERR_INVALID_ARG;  // (hdv-v1: step(None))
  hipStream_t s = (hipStream_t)stream;
  if (h->envp && out->trace) {  // (the trace-carrying kernels read the uniform values: refused, never a quiet fall-back)
    snprintf(h->err, sizeof h->err, "mm_step: no trace while per-env parameters are set (mm_set_env_params)");
    return MM_ERR_INVALID_ARG;
  }
  if (out->trace) {
    // NaN = "sub-step did not run"; 0xFF bytes are a NaN pattern
    hipError_t rc = hipMemsetAsync(out->trace, 0xFF, (size_t)3 * MM_T_COUNT * h->E * h->N * sizeof(double), s);
    if (rc != hipSuccess) return hip_fail(h, rc, "trace memset");
  }
  if (h->cfg.env_kind == MM_ENV_HDV_V1) {  // every vehicle an IDM / MOBIL HDV (mm_idm.o)
    mm_launch_step_idm(h, step_group(h), out, s);
  } else if (steps_split(h)) {  // interior-point mode, CAV-only: phase kernels + sweep kernels (SweepBuf)
    if (!h->sweep_mem) { snprintf(h->err, sizeof h->err, "mm_step: the hand-off planes of the split interior-point step are missing"); return MM_ERR_DEVICE; }
    mm_launch_step_split(h, step_group(h), actions, out, s);
  } else if (carries_pose(h) && !h->pose_mem) {
    snprintf(h->err, sizeof h->err, "mm_step: the carried pose planes are missing");
    return MM_ERR_DEVICE;
  } else if (h->envp) {  // per-env eta / tau / headway_time: the PENV kernels (mm_penv.o, mm_penv_ipm.o), fused at every batch size
    mm_launch_step_penv(h, step_group(h), actions, out, s);
  } else {
#define MM_STEP_CASE(GG) launch_step_g<GG>(h, actions, out, s)
#define MM_LANES_CASE(GG) mm_launch_step_lanes(h, GG, actions, out, s)
    MM_FOR_GROUP(step_group(h), MM_STEP_CASE, MM_LANES_CASE);
#undef MM_STEP_CASE
#undef MM_LANES_CASE
  }
  if (h->metrics && !h->metrics_deferred) launch_metrics_flush(h, s, 0);  // fold this launch's per-wave partials into the caller's 8 doubles (same stream: ordered)
  hipError_t rc = hipGetLastError();
  return rc == hipSuccess ? MM_OK : hip_fail(h, rc, "step launch");
}

template <int G, bool IPM>
static void launch_shield_gi(MMHandle h, const double *as, const double *aa, double *ss, double *sa, uint8_t *stt,
                             double *mg, double *hw, hipStream_t s) {
  const long long threads = (long long)h->E * G;
  const unsigned grid = (unsigned)((threads + 255) / 256);
  const int sh = h->cfg.env_kind == MM_ENV_V1 ? h->cfg.shield : MM_SHIELD_NONE;
  DevCfg dc = dev_cfg(h);
  dc.err = h->dev_err + MM_LW_SHIELD;  // this entry reports synchronously from its own latch word
  if (sh == MM_SHIELD_MASS)
    hipLaunchKernelGGL((shield_kernel<G, MM_SHIELD_MASS, IPM>), dim3(grid), dim3(256), 0, s, dc, dev_state(h), as, aa, ss, sa, stt, mg, hw);
  else if (sh == MM_SHIELD_HSS)
    hipLaunchKernelGGL((shield_kernel<G, MM_SHIELD_HSS, IPM>), dim3(grid), dim3(256), 0, s, dc, dev_state(h), as, aa, ss, sa, stt, mg, hw);
  else
    hipLaunchKernelGGL((shield_kernel<G, MM_SHIELD_NONE, false>), dim3(grid), dim3(256), 0, s, dc, dev_state(h), as, aa, ss, sa, stt, mg, hw);
}
template <int G>
static void launch_shield_g(MMHandle h, const double *as, const double *aa, double *ss, double *sa, uint8_t *stt,
                            double *mg, double *hw, hipStream_t s) {
  if (h->cfg.qp_solver == MM_QP_IPM) launch_shield_gi<G, true>(h, as, aa, ss, sa, stt, mg, hw, s);
  else launch_shield_gi<G, false>(h, as, aa, ss, sa, stt, mg, hw, s);
}
extern "C" int32_t mm_shield_actions(MMHandle h, const double *act_steer, const double *act_acc, double *safe_steer,
                                     double *safe_acc, uint8_t *status, double *margin, double *headway, MMStream stream) {
  if (!h || !act_steer || !act_acc || !safe_steer || !safe_acc) return MM_ERR_INVALID_ARG;
  if (h->envp) {  // (the stand-alone shield kernel reads the uniform values: refused, never a quiet fall-back)
    snprintf(h->err, sizeof h->err, "mm_shield_actions: not available while per-env parameters are set (mm_set_env_params)");
    return MM_ERR_INVALID_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
#define MM_SHIELD_CASE(GG) launch_shield_g<GG>(h, act_steer, act_acc, safe_steer, safe_acc, status, margin, headway, s)
  MM_FOR_GROUP(group_size(h->N), MM_SHIELD_CASE, MM_NO_GROUP);
#undef MM_SHIELD_CASE
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return hip_fail(h, rc, "shield launch");
  // the reference call raises check_bounds' ValueError synchronously (only the IPM iterate can leave the bounds)
  return h->cfg.qp_solver == MM_QP_IPM ? poll_latch(h, MM_LW_SHIELD, stream) : MM_OK;
}

extern "C" int32_t mm_shield_qp(MMHandle h, int32_t n, const double *G, const double *hvec, const int32_t *rows,
                                int32_t solver, double *u_out, uint8_t *status, int32_t *iters, MMStream stream) {
  if (!h || n < 0 || (solver != MM_QP_EXACT && solver != MM_QP_IPM)) return MM_ERR_INVALID_ARG;
  if (n == 0) return MM_OK;
  if (!G || !hvec || !rows || !u_out) return MM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(qp_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, G, hvec, rows, (int)solver, u_out,
                     status, iters, h->dev_err + MM_LW_QP);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return hip_fail(h, rc, "qp launch");
  return poll_latch(h, MM_LW_QP, stream);
}

// diagnostics: element-wise mm_math evaluation (CPU/GPU bit-equality tests)
__global__ void math_kernel(int fn, int n, const double *__restrict__ x, const double *__restrict__ x2,
                            double *__restrict__ y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = x[i], r;
  switch (fn) {
    case 0: r = mmm_sin(v); break;
    case 1: r = mmm_cos(v); break;
    case 2: r = mmm_tan(v); break;
    case 3: r = mmm_atan(v); break;
    case 4: r = mmm_asin(v); break;
    case 5: r = mmm_exp(v); break;
    case 6: r = mmm_log(v); break;
    case 7: r = sqrt(v); break;
    case 9: r = div_c(v, x2[i], 1.0 / x2[i]); break;
    default: r = v / x2[i]; break;
  }
  y[i] = r;
}
extern "C" int32_t mm_math_eval(int32_t fn, int32_t n, const double *x, const double *x2, double *y,
                                MMStream stream) {
  if (fn < 0 || fn > 9 || n <= 0) return MM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(math_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, fn, n, x, x2, y);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

// diagnostics: the step kernel's geometric device functions on stand-alone rows (include/mm_abi.h: mm_geom_eval)
__global__ void geom_kernel(int fn, int n, const double *__restrict__ in, double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (fn == MM_GEOM_POSE) {
    const double x = in[i * 3 + 0], y = in[i * 3 + 1], h = in[i * 3 + 2];
    double *o = out + (long long)i * 19;
    o[0] = closest_lane(x, y, h);
    for (int l = 0; l < 6; l++) {
      o[1 + l] = next_lane(l, x, y);
      o[7 + l] = lane_reachable(l, x, y) ? 1.0 : 0.0;
      o[13 + l] = lane_after_end(l, x) ? 1.0 : 0.0;
    }
  } else if (fn == MM_GEOM_STEER) {
    const double *r = in + (long long)i * 5;
    out[i] = steering_control(r[0], r[1], r[2], r[3], (int)r[4]);
  } else if (fn == MM_GEOM_RECT) {
    const double *r = in + (long long)i * 6;
    double *o = out + (long long)i * 4;
    const double dx = r[3] - r[0], dy = r[4] - r[1];
    const bool near = !((dx * dx + dy * dy) > kU5);  // the step kernel's form of `norm > LENGTH`
    const bool t_v = near && boxes_may_touch(dx, dy, r[2], r[5], 0.9 * kVehLength / 2, 0.9 * kVehWidth / 2);
    const bool t_o = near && boxes_may_touch(dx, dy, r[2], 0.0, 0.9 * 2.0 / 2, 0.9 * 2.0 / 2);
    const bool full_v = rects_intersect(r[0], r[1], r[2], r[3], r[4], kVehLength, kVehWidth, r[5]);
    const bool full_o = rects_intersect(r[0], r[1], r[2], r[3], r[4], 2.0, 2.0, 0.0);
    o[0] = (t_v && full_v) ? 1.0 : 0.0; o[1] = (t_o && full_o) ? 1.0 : 0.0;
    o[2] = full_v ? 1.0 : 0.0; o[3] = full_o ? 1.0 : 0.0;
  } else if (fn == MM_GEOM_DIV) {
    const double x = in[i * 2 + 0], d = in[i * 2 + 1];
    double *o = out + (long long)i * 4;
    const double y = rcp_rn(d);
    const bool ok = rcp_ok(d);
    o[0] = div_g(x, d, y, ok);
    o[1] = rcp_g(d, y, ok);
    const bool integral = fabs(d) <= 1e9 && d == (double)(int)d;
    o[2] = integral ? div_n(x, (int)d, integral) : __builtin_nan("");
    o[3] = div_g(x, d, y, ok, false);  // a lane that does not need its quotient never sends the wave to the plain division
  } else {
    out[i] = speed_to_index(in[i]);
  }
}
extern "C" int32_t mm_geom_eval(int32_t fn, int32_t n, const double *in, double *out, MMStream stream) {
  if (fn < MM_GEOM_POSE || fn > MM_GEOM_DIV || n <= 0 || !in || !out) return MM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(geom_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, fn, n, in, out);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

// marl/mappo.py:220-236 exploration_action / action for a batch (include/mm_abi.h): softmax -> inverse-CDF
// categorical sample, one thread per agent; HBM-bound by construction (4 n_a + 4 bytes per agent).
__global__ __launch_bounds__(256) void sample_kernel(const float *__restrict__ logp, long long n, int n_a, uint64_t seed,
                                                     const uint64_t *__restrict__ counter, int32_t *__restrict__ actions) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t ctr = *counter;
  double cdf[8], acc = 0;
#pragma unroll
  for (int k = 0; k < 8; k++)
    if (k < n_a) { acc = acc + mmm_exp((double)logp[i * n_a + k]); cdf[k] = acc; }
  uint32_t o[4];
  philox4x32((uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32) ^ 0x53414D50u,
             (uint32_t)seed, (uint32_t)(seed >> 32), o);
  const double u = u53(o[0], o[1]);
  int a = 0;
#pragma unroll
  for (int k = 0; k < 8; k++)
    if (k < n_a) a += (cdf[k] / acc <= u) ? 1 : 0;  // searchsorted(cdf / cdf[-1], u, "right")
  actions[i] = a < n_a - 1 ? a : n_a - 1;
}
__global__ void bump_kernel(uint64_t *counter) { *counter += 1; }
extern "C" int32_t mm_sample_actions(const float *logp, int64_t n, int32_t n_a, uint64_t seed, uint64_t *counter,
                                     int32_t *actions, MMStream stream) {
  if (!logp || !actions || !counter || n < 0 || n_a < 1 || n_a > 8) return MM_ERR_INVALID_ARG;
  if (n == 0) return MM_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, logp, (long long)n, (int)n_a, seed, counter, actions);
  hipLaunchKernelGGL(bump_kernel, dim3(1), dim3(1), 0, s, counter);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

// marl/mappo.py:147-156,364-370: reward scaling + discounted returns of a whole rollout, one thread per agent, T values
// each, consecutive threads on consecutive addresses at every t (include/mm_abi.h: mm_discount_returns)
__global__ __launch_bounds__(256) void discount_kernel(const double *rewards, const uint8_t *__restrict__ dones,
                                                       const double *__restrict__ final_value, int T, long long n_env, int n_agent,
                                                       double gamma, double scale, double *returns) {
  const long long A = n_env * n_agent;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A) return;
  const long long e = i / n_agent;
  double running = final_value[i];
  for (int t = T - 1; t >= 0; t--) {
    double r = rewards[(long long)t * A + i];
    if (scale > 0) r = r / scale;
    if (dones[(long long)t * n_env + e]) running = 0.0;
    running = running * gamma + r;
    returns[(long long)t * A + i] = running;
  }
}
extern "C" int32_t mm_discount_returns(const double *rewards, const uint8_t *dones, const double *final_value, int32_t T,
                                       int64_t n_env, int32_t n_agent, double gamma, double reward_scale, double *returns,
                                       MMStream stream) {
  if (!rewards || !dones || !final_value || !returns || T < 0 || n_env < 0 || n_agent < 1) return MM_ERR_INVALID_ARG;
  const long long A = (long long)n_env * n_agent;
  if (A == 0 || T == 0) return MM_OK;
  hipLaunchKernelGGL(discount_kernel, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rewards, dones,
                     final_value, (int)T, (long long)n_env, (int)n_agent, gamma, reward_scale, returns);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

// ------------------------------------------------------------------------------------------------
// mm_policy_act: the actor forward of the rollout loop fused with the sampling above
// (marl/single_agent/Model_common.py:5-22 ActorNetwork: n_s -> 128 -> 128 -> n_a, ReLU, log-softmax;
// marl/mappo.py:220-236).  The one GEMM-shaped piece of the path, so it runs on the matrix cores:
// f32-input MFMA (v_mfma_f32_32x32x2_f32, exact fp32 products and sums).
//
// Orientation: every layer is computed transposed, H_out^T [feature x agent] = W [out x in] . H_in^T, one
// wave per 32 agents.  A 32x32 accumulator tile then has its agent on the lane and its features in the 16
// registers, which is exactly the B-operand layout of the next layer's MFMAs (k = feature): activations
// never leave the register file -- no LDS round trip, no transposes.  Lane (j = l & 31, h = l >> 5) holds
// features row(r, h) = (r & 3) + 8 (r >> 2) + 4 h of a tile in register r, so k-step s of a 32-feature
// chunk pairs feature row(s, 0) (lanes h = 0) with row(s, 1) (lanes h = 1); the weight fragments are
// staged once per workgroup in LDS in that order (84 KB), read back as one conflict-free float4 per four
// MFMAs.  Layer 3 (n_a <= 8 outputs) would waste 27/32 of a tile: done with 64 FMAs per output per lane
// plus one cross-half add.  Then log-softmax (fp32) and the inverse-CDF sample (fp64), written by h = 0.
// ------------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kPolHidden = 128;
MM_DEV int frag_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
constexpr int kPolThreads = 512;  // 8 waves = 2 per SIMD: one wave's VALU tail (layer 3, sampling) overlaps the other's MFMAs
__global__ __launch_bounds__(kPolThreads) void policy_kernel(const float *__restrict__ obs, long long n, int n_s,
                                                        const float *__restrict__ W1, const float *__restrict__ b1,
                                                        const float *__restrict__ W2, const float *__restrict__ b2,
                                                        const float *__restrict__ W3, const float *__restrict__ b3, int n_a,
                                                        uint64_t seed, const uint64_t *__restrict__ counter,
                                                        int32_t *__restrict__ actions, float *__restrict__ logp_out) {
  __shared__ float4 sW1[4][4][64];    // [out tile][k-step / 4][lane] : 16 KB
  __shared__ float4 sW2[4][16][64];   // 64 KB
  __shared__ float sW3[8][kPolHidden];
  __shared__ float sB1[kPolHidden], sB2[kPolHidden], sB3[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  // ---- stage the weights in MFMA A-fragment order: A[i = l & 31][k = l >> 5] of step s is W[32 m + i][k(s, h)]
  for (int t = tid; t < 4 * 4 * 64; t += kPolThreads) {
    const int l = t & 63, q = (t >> 6) & 3, m = t >> 8;
    float w[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = frag_row(4 * q + u, l >> 5);
      w[u] = k < n_s ? W1[(32 * m + (l & 31)) * n_s + k] : 0.0f;
    }
    sW1[m][q][l] = make_float4(w[0], w[1], w[2], w[3]);
  }
  for (int t = tid; t < 4 * 16 * 64; t += kPolThreads) {
    const int l = t & 63, q = (t >> 6) & 15, m = t >> 10;
    float w[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int s = 4 * q + u;  // k-step 0..63: chunk s >> 4, step in chunk s & 15
      w[u] = W2[(32 * m + (l & 31)) * kPolHidden + 32 * (s >> 4) + frag_row(s & 15, l >> 5)];
    }
    sW2[m][q][l] = make_float4(w[0], w[1], w[2], w[3]);
  }
  for (int t = tid; t < 8 * kPolHidden; t += kPolThreads) sW3[t / kPolHidden][t % kPolHidden] = (t / kPolHidden) < n_a ? W3[t] : 0.0f;
  if (tid < kPolHidden) { sB1[tid] = b1[tid]; sB2[tid] = b2[tid]; }
  if (tid < 8) sB3[tid] = tid < n_a ? b3[tid] : 0.0f;
  __syncthreads();
  const uint64_t ctr = *counter;
  const long long ntiles = (n + 31) / 32;
  constexpr int kWaves = kPolThreads / 64;
  for (long long tile = (long long)blockIdx.x * kWaves + wave; tile < ntiles; tile += (long long)gridDim.x * kWaves) {
    // the weight fragments are tile-invariant: without this the compiler hoists all 80 float4 LDS reads out of
    // the persistent loop (320 registers) and spills the activations
    asm volatile("" ::: "memory");
    const long long ag = tile * 32 + j;
    const bool live = ag < n;
    float xk[16];  // B operand of layer 1: x[agent j][k(s, h)]
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const int k = frag_row(s, h);
      xk[s] = (live && k < n_s) ? obs[ag * n_s + k] : 0.0f;
    }
    f32x16 h1[4], h2[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; r++) acc[r] = sB1[32 * m + frag_row(r, h)];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const float4 a = sW1[m][q][lane];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, xk[4 * q + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, xk[4 * q + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, xk[4 * q + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, xk[4 * q + 3], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; r++) h1[m][r] = fmaxf(acc[r], 0.0f);
    }
#pragma unroll
    for (int m = 0; m < 4; m++) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; r++) acc[r] = sB2[32 * m + frag_row(r, h)];
#pragma unroll
      for (int c = 0; c < 4; c++) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const float4 a = sW2[m][4 * c + q][lane];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, h1[c][4 * q + 0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, h1[c][4 * q + 1], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, h1[c][4 * q + 2], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, h1[c][4 * q + 3], acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; r++) h2[m][r] = fmaxf(acc[r], 0.0f);
    }
    // ---- layer 3 + log-softmax + sample
    float logit[8];
#pragma unroll
    for (int o = 0; o < 8; o++) {
      float p = 0.0f;
      if (o < n_a) {
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
          for (int r = 0; r < 16; r++) p = fmaf(h2[m][r], sW3[o][32 * m + frag_row(r, h)], p);
      }
      p = p + __shfl_xor(p, 32, 64);
      logit[o] = o < n_a ? p + sB3[o] : -INFINITY;
    }
    float mx = logit[0];
#pragma unroll
    for (int o = 1; o < 8; o++) mx = fmaxf(mx, logit[o]);
    float se = 0.0f;
#pragma unroll
    for (int o = 0; o < 8; o++) se += (o < n_a) ? expf(logit[o] - mx) : 0.0f;
    // log-softmax as (logit - mx) - log(sum), torch's order: logit - (mx + log(sum)) rounds the normaliser at ulp(mx) and
    // shifts a whole row by up to ulp(max |logit|) / 2 (4e-6 at |logit| ~ 100: logsumexp(logp) is then no longer 0 to 1e-6)
    const float lg = logf(se);
    if (live && h == 0) {
      double cdf[8], acc = 0;
#pragma unroll
      for (int o = 0; o < 8; o++) {
        const float lp = (logit[o] - mx) - lg;
        if (o < n_a) {
          if (logp_out) logp_out[ag * n_a + o] = lp;
          acc = acc + mmm_exp((double)lp);
          cdf[o] = acc;
        }
      }
      uint32_t w4[4];
      philox4x32((uint32_t)ag, (uint32_t)((uint64_t)ag >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32) ^ 0x53414D50u,
                 (uint32_t)seed, (uint32_t)(seed >> 32), w4);
      const double u = u53(w4[0], w4[1]);
      int a = 0;
#pragma unroll
      for (int o = 0; o < 8; o++)
        if (o < n_a) a += (cdf[o] / acc <= u) ? 1 : 0;
      actions[ag] = a < n_a - 1 ? a : n_a - 1;
    }
  }
}
extern "C" int32_t mm_policy_act(const float *obs, int64_t n, int32_t n_s, const float *W1, const float *b1, const float *W2,
                                 const float *b2, const float *W3, const float *b3, int32_t hidden, int32_t n_a, uint64_t seed,
                                 uint64_t *counter, int32_t *actions, float *logp, MMStream stream) {
  if (!obs || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !counter || !actions) return MM_ERR_INVALID_ARG;
  if (hidden == 512)  // the reference's other actor size: its own kernel (mm_policy_wide.hip), the same contract
    return mm_policy_wide_act(obs, n, n_s, W1, b1, W2, b2, W3, b3, hidden, n_a, seed, counter, actions, logp, stream);
  if (n < 0 || n_s < 1 || n_s > 32 || hidden != kPolHidden || n_a < 1 || n_a > 8) return MM_ERR_INVALID_ARG;
  if (n == 0) return MM_OK;
  hipStream_t s = (hipStream_t)stream;
  const long long ntiles = (n + 31) / 32;
  constexpr int kW = kPolThreads / 64;
  const unsigned grid = (unsigned)(ntiles < kW * 256 ? (ntiles + kW - 1) / kW : 256);  // one persistent workgroup per CU
  hipLaunchKernelGGL(policy_kernel, dim3(grid), dim3(kPolThreads), 0, s, obs, (long long)n, (int)n_s, W1, b1, W2, b2, W3, b3, (int)n_a,
                     seed, counter, actions, logp);
  hipLaunchKernelGGL(bump_kernel, dim3(1), dim3(1), 0, s, counter);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}

#ifdef MM_STAMPS
extern "C" int32_t mm_debug_read_sweep_stamps(unsigned long long *out8, int32_t reset) {
  static unsigned long long host[4096 * 8];
  hipError_t rc = hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps_s), sizeof host);
  for (int k = 0; k < 8; k++) out8[k] = 0;
  for (int w = 0; w < 4096; w++)
    for (int k = 0; k < 8; k++) out8[k] += host[w * 8 + k];
  if (rc == hipSuccess && reset) {
    memset(host, 0, sizeof host);
    rc = hipMemcpyToSymbol(HIP_SYMBOL(g_stamps_s), host, sizeof host);
  }
  return rc == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
extern "C" int32_t mm_debug_read_stamps(unsigned long long *out16, int32_t reset) {
  static unsigned long long *host = nullptr;
  if (!host) host = (unsigned long long *)malloc(sizeof(unsigned long long) * MM_STAMP_WAVES * 16);
  hipError_t rc = hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps_w), sizeof(unsigned long long) * MM_STAMP_WAVES * 16);
  for (int k = 0; k < 16; k++) out16[k] = 0;
  for (long long w = 0; w < MM_STAMP_WAVES; w++)
    for (int k = 0; k < 16; k++) out16[k] += host[w * 16 + k];
  if (rc == hipSuccess && reset) {
    memset(host, 0, sizeof(unsigned long long) * MM_STAMP_WAVES * 16);
    rc = hipMemcpyToSymbol(HIP_SYMBOL(g_stamps_w), host, sizeof(unsigned long long) * MM_STAMP_WAVES * 16);
  }
  return rc == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
// the wave records of the last step_kernel launch, raw: out[n_waves][MM_REC_WORDS] (n_waves <= MM_REC_WAVES)
extern "C" int32_t mm_debug_read_wave_records(unsigned long long *out, int32_t n_waves) {
  if (!out || n_waves <= 0 || n_waves > MM_REC_WAVES) return MM_ERR_INVALID_ARG;
  hipError_t rc = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_rec), sizeof(unsigned long long) * MM_REC_WORDS * (size_t)n_waves);
  return rc == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
// out32[k], k = slot - 16: the cycle sum (the slots of mm_cs_is_cycles) or the lanes counted; out32[16 + k]: the waves counted
extern "C" int32_t mm_debug_read_cand_stamps(unsigned long long *out32, int32_t reset) {
  static unsigned long long *host = nullptr;
  if (!host) host = (unsigned long long *)malloc(sizeof(unsigned long long) * MM_STAMP_WAVES * 16);
  hipError_t rc = hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps_c), sizeof(unsigned long long) * MM_STAMP_WAVES * 16);
  for (int k = 0; k < 32; k++) out32[k] = 0;
  for (long long w = 0; w < MM_STAMP_WAVES; w++)
    for (int k = 0; k < 16; k++) {
      const unsigned long long x = host[w * 16 + k];
      if (mm_cs_is_cycles(k + 16)) { out32[k] += x; continue; }
      out32[k] += x & 0xFFFFFFFFull;
      out32[16 + k] += x >> 32;
    }
  if (rc == hipSuccess && reset) {
    memset(host, 0, sizeof(unsigned long long) * MM_STAMP_WAVES * 16);
    rc = hipMemcpyToSymbol(HIP_SYMBOL(g_stamps_c), host, sizeof(unsigned long long) * MM_STAMP_WAVES * 16);
  }
  return rc == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
#endif
