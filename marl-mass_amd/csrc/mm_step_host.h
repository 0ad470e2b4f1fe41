// mm_step_host.h -- host side of the step library, shared by its ten objects (Makefile): the handle, what a configuration
// steps with, the launch templates that instantiate the kernels of mm_kernels.hip, and the declarations of the launchers the
// objects call across each other.  Each source defines its own launchers and so decides which kernels its object holds:
//   mm_main.hip                          the C ABI, reset / observe, the mm_step dispatch, the CAV-only exact-mode step kernels
//   mm_general.hip                       the step kernels that carry HDVs (IDM / MOBIL) and steer_vel
//   mm_ipm.hip                           the fused interior-point (MM_QP_IPM) step kernels
//   mm_lanes.hip / mm_lanes_ipm.hip      the exact-mode / interior-point step kernels in the 6- / 12-lane rotation layouts
//   mm_split.hip / mm_split_general.hip  the split interior-point step, CAV-only / general
//   mm_idm.hip                           reset and step of merge-multi-agent-hdv-v1
//   mm_penv.hip / mm_penv_ipm.hip        the exact-mode / interior-point step kernels with per-env eta / tau / headway_time
// mm_step_all.hip includes all ten: the single-object form of the tuning and stamps builds.
//
// Tuning short-cuts (`make tuning EXTRA="-DMM_ONLY_G=8 -DMM_ONLY_MIXED=false"`: one group size compiles in about a minute).
// They are spelled in this header and nowhere else, and the product build defines none of them:
//   MM_ONLY_G=g       the one group size that is compiled: step_group() returns it, MM_FOR_GROUP expands it alone
//   MM_NO_LANES       power-of-two groups only (step_group())
//   MM_ONLY_MIXED=b   kOnlyMixed: needs_general() is the constant b and the other kind's step kernels are not built; kOnlyIpm: the
//                     fused kernels are the exact-mode ones, or with MM_ONLY_IPM as well the interior-point ones
//   MM_ONLY_SHIELD=s  launch_step_m() launches v1 with shield s, whatever the configuration
// A launch of a kernel that a short-cut left out does nothing.
#pragma once
#include "mm_kernels.hip"

static int group_size(int N) { return N <= 2 ? 2 : (N <= 4 ? 4 : (N <= 8 ? 8 : 16)); }

struct MMHandle_ : MMHandleHead {  // cfg, E, N, device, state, lay, first_env: mm_handle.h
  double *metrics;          // caller's 8 doubles (mm_set_metrics_buffer) or NULL
  double *metrics_partial;  // [waves of a step launch][8], device, owned by the handle
  int metrics_deferred;     // mm_defer_metrics: the partials accumulate across launches, folded by mm_flush_metrics only
  // device error latches (MM_LATCH_* bits), hipMalloc'd at create.  One word per entry point that reports synchronously, so
  // that a condition latched by an un-polled mm_step cannot fail a later, valid mm_shield_qp / mm_shield_actions call (or be
  // consumed by it): [MM_LW_STEP] mm_step -> mm_poll_errors, [MM_LW_QP] mm_shield_qp, [MM_LW_SHIELD] mm_shield_actions
  int *dev_err;
  // hand-off planes of the split interior-point step (SweepBuf): allocated by mm_create / mm_set_config when the
  // configuration steps that way (shielded v1, qp_solver = MM_QP_IPM, CAV-only), never inside mm_step
  SweepBuf sweep;
  void *sweep_mem;
  // derived pose values carried from launch to launch (PoseBuf): allocated by mm_create / mm_set_config for the shielded v1
  // configurations, whose exact-mode CAV-only step kernels read and write them; never inside mm_step
  PoseBuf pose;
  void *pose_mem;
  int n_simd;  // SIMDs of the handle's device (4 per CU), read at mm_create
  const double *envp;  // mm_set_env_params: the caller's [MM_ENVP_COUNT][E] planes, or NULL
  char err[256];
};
// what the per-env planes exist for: the shielded v1 step (include/mm_env_params.h)
static bool envp_scope(const MMConfig *c) { return c->env_kind == MM_ENV_V1 && (c->shield == MM_SHIELD_HSS || c->shield == MM_SHIELD_MASS); }
// -1: the build holds both kinds of kernel and the configuration decides; 0 / 1: it holds one kind, which every batch gets
#ifdef MM_ONLY_MIXED
constexpr int kOnlyMixed = MM_ONLY_MIXED ? 1 : 0;
#else
constexpr int kOnlyMixed = -1;
#endif
#if defined(MM_ONLY_IPM)
constexpr int kOnlyIpm = 1;
#elif defined(MM_ONLY_MIXED)
constexpr int kOnlyIpm = 0;
#else
constexpr int kOnlyIpm = -1;
#endif
template <bool MIXED> constexpr bool kMixedBuilt = kOnlyMixed < 0 || MIXED == (kOnlyMixed == 1);
// (hdv-v1 has one kind of step kernel and keeps it)
template <int KIND, bool MIXED, bool IPM> constexpr bool kFusedBuilt = kIdm<KIND> || (kMixedBuilt<MIXED> && (kOnlyIpm < 0 || IPM == (kOnlyIpm == 1)));
static bool needs_general(const MMHandle_ *h) {  // HDVs can appear, or steer_vel lateral control: the kernels that carry IDM / MOBIL
  if (kOnlyMixed >= 0) return kOnlyMixed == 1;
  return h->cfg.env_kind == MM_ENV_HDV_V1 || h->cfg.n_hdv > 0 || (h->cfg.traffic_density > 0 && h->cfg.mixed_traffic != 0) ||
         (h->cfg.env_kind == MM_ENV_V1 && h->cfg.lateral_control == MM_LATERAL_STEER_VEL);
}
static bool fused_ipm(const MMHandle_ *h) {  // the fused step of this configuration runs the interior-point kernels
  if (kOnlyIpm >= 0) return kOnlyIpm == 1;
  return h->cfg.env_kind == MM_ENV_V1 && h->cfg.shield != MM_SHIELD_NONE && h->cfg.qp_solver == MM_QP_IPM;
}
// The interior-point mode of a CAV-only shielded batch steps as phase kernels + sweep kernels (SweepBuf above) once the
// batch is large enough for it.  The split step takes as long as its slowest env needs for its QP chain, almost independent of
// the batch (one lane per env, one wave per SIMD up to 65 536 envs); the fused kernel iterates with ~8 of 64 lanes busy but a
// small batch leaves the chip's other lanes idle anyway.  Measured at N = 8 MASS (ms per step, fused / split; tools/split_crossover.sh):
// 8 192 envs 1.12 / 1.31, 12 288 envs 1.43 / 1.33, 16 384 envs 1.46 / 1.36, 32 768 envs 2.46 / 1.54; N = 4 HSS: 4 096 envs 0.30 /
// 0.64, 16 384 envs 0.32 / 0.73.  Crossover = more than one fused wave per SIMD for the 8- and 16-lane groups (long chains per
// env), more than two for the 2- and 4-lane groups.  debug_flags bit2 keeps the fused kernel, bit3 forces the split step at any size
// (validation / A-B timing: same results either way).
static bool steps_split(const MMHandle_ *h) {
  if (!(h->cfg.env_kind == MM_ENV_V1 && h->cfg.shield != MM_SHIELD_NONE && h->cfg.qp_solver == MM_QP_IPM)) return false;
  if (h->envp) return false;  // per-env parameters: the sweep kernel reads the uniform values, the fused kernel steps such a batch
  if (h->cfg.debug_flags & 4) return false;
  if (h->cfg.debug_flags & 8) return true;
  const int g = h->N <= 2 ? 2 : (h->N <= 4 ? 4 : (h->N <= 8 ? 8 : 16));
  return (long long)h->E * g / 64 > (g >= 8 ? 1ll : 2ll) * (h->n_simd > 0 ? h->n_simd : 1024);
}

// waves one step launch starts (launch_step_t rounds the grid up to whole MM_STEP_BLOCK-thread blocks): every one of them
// stores its 64-byte slot of the metrics partial buffer
// waves of a step launch in the power-of-two layout: the size of the metrics partial buffer (a launch in a rotation layout
// has fewer waves -- more envs per wave -- never more)
static long long step_launch_waves(const MMHandle h) {
  const long long threads = (long long)h->E * group_size(h->N);
  return (threads + MM_STEP_BLOCK - 1) / MM_STEP_BLOCK * (MM_STEP_BLOCK / 64);
}
// Lanes per env group of the step launch: batches of 5..6 / 9..12 vehicles run the 6- / 12-lane rotation layouts (kPow2
// above: 10 / 5 envs per wave instead of 8 / 4, 5 / 11 partners per loop instead of 7 / 15), the others power-of-two groups.
static int step_group(const MMHandle h) {
  const int g = group_size(h->N);
#if defined(MM_ONLY_G)
  (void)g;
  return MM_ONLY_G;
#elif defined(MM_NO_LANES)
  return g;
#else
  if (h->cfg.debug_flags & 2) return g;  // (debug_flags bit1: validation / A-B timing against the power-of-two groups)
  if (h->N == 5 || h->N == 6) return 6;
  if (h->N >= 9 && h->N <= 12) return 12;
  return g;
#endif
}
static long long step_launch_waves_now(const MMHandle h) {
  const int g = step_group(h);
  if ((g & (g - 1)) == 0) return step_launch_waves(h);
  const long long epw = 64 / g;
  return (h->E + epw - 1) / epw;
}
// MM_FOR_GROUP(g, POW2, ROT): the statement POW2(G) for the compiled power-of-two group size G that equals g, ROT(G) for the
// compiled rotation layout (6, 12); a dispatch that has no rotation form passes MM_NO_GROUP for it
#define MM_NO_GROUP(G) (void)0
#ifdef MM_ONLY_G
#define MM_FOR_GROUP(g, POW2, ROT) do { (void)(g); POW2(MM_ONLY_G); } while (0)
#else
#define MM_FOR_GROUP(g, POW2, ROT) \
  switch (g) {                     \
    case 2: POW2(2); break;        \
    case 4: POW2(4); break;        \
    case 6: ROT(6); break;         \
    case 8: POW2(8); break;        \
    case 12: ROT(12); break;       \
    case 16: POW2(16); break;      \
    default: break;                \
  }
#endif

// The launchers the step objects call across each other, each defined in the source of its name (mm_general.hip ...
// mm_penv_ipm.hip; the two hdv-v1 ones in mm_idm.hip).  `g` is step_group(h).
void mm_launch_step_general(MMHandle h, const int32_t *actions, const MMStepOut *out, hipStream_t s);
void mm_launch_step_ipm(MMHandle h, const int32_t *actions, const MMStepOut *out, hipStream_t s);
void mm_launch_step_lanes(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s);
void mm_launch_step_lanes_ipm(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s);
void mm_launch_step_split(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s);
void mm_launch_step_split_general(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s);
void mm_launch_step_penv(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s);
void mm_launch_step_penv_ipm(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s);
void mm_launch_reset_idm(MMHandle h, int mode, const uint8_t *mask, const uint64_t *seeds, void *obs, uint8_t *avail, hipStream_t s);
void mm_launch_step_idm(MMHandle h, int g, const MMStepOut *out, hipStream_t s);

static DevCfg dev_cfg(const MMHandle h) {
  const MMConfig &c = h->cfg;
  DevCfg d;
  d.env_kind = c.env_kind; d.shield = c.env_kind == MM_ENV_V1 ? c.shield : MM_SHIELD_NONE;
  d.nsub = c.simulation_frequency / c.policy_frequency; d.T = c.duration * c.policy_frequency;
  d.action_masking = c.action_masking; d.auto_reset = c.auto_reset; d.obs_f64 = c.obs_f64; d.N = h->N; d.E = h->E;
  d.debug_flags = (c.debug_flags & ~(1 << kMetricsAccBit)) | (h->metrics_deferred ? (1 << kMetricsAccBit) : 0); d.n_hdv = c.n_hdv;
  d.dt = 1.0 / c.simulation_frequency;
  d.collision_reward = c.collision_reward; d.high_speed_reward = c.high_speed_reward;
  d.headway_cost = c.headway_cost; d.headway_time = c.headway_time; d.merging_lane_cost = c.merging_lane_cost;
  d.rs_lo = c.reward_speed_lo; d.rs_hi = c.reward_speed_hi; d.eta = c.cbf_eta; d.tau = c.cbf_tau;
  d.inv_dt = 1.0 / d.dt; d.rs_span = d.rs_hi - d.rs_lo; d.rs_ispan = 1.0 / d.rs_span;
  d.rs_span2 = (d.rs_lo + (d.rs_hi - d.rs_lo) / 2) - d.rs_lo; d.rs_ispan2 = 1.0 / d.rs_span2;  // mrew, collaborating
  d.agent_reward = c.env_kind == MM_ENV_V1 ? c.agent_reward : 0;
  d.steer_vel = (c.env_kind == MM_ENV_V1 && c.lateral_control == MM_LATERAL_STEER_VEL) ? 1 : 0;
  d.err = h->dev_err + MM_LW_STEP;
  d.traffic_density = c.traffic_density; d.mixed_traffic = c.mixed_traffic; d.num_cav = c.num_cav;
  d.envp = h->envp;
  return d;
}
static DevState dev_state(const MMHandle h) {
  DevState s;
  s.F = (double *)(h->state + h->lay.f64_offset); s.B = h->state + h->lay.u8_offset;
  s.I = (int32_t *)(h->state + h->lay.env_offset); s.seeds = (uint64_t *)(h->state + h->lay.seed_offset);
  s.A = (long long)h->E * h->N; s.E = h->E; s.N = h->N;
  return s;
}
template <int G, int KIND>
static void launch_reset_t(MMHandle h, int mode, const uint8_t *mask, const uint64_t *seeds, void *obs,
                           uint8_t *avail, hipStream_t s) {
  const long long threads = (long long)h->E * G;
  const unsigned grid = (unsigned)((threads + 255) / 256);
  hipLaunchKernelGGL((reset_kernel<G, KIND>), dim3(grid), dim3(256), 0, s, dev_cfg(h), dev_state(h), mode, mask,
                     seeds, obs, avail);
}
template <int G, int KIND, int SHIELD, bool MIXED, bool IPM = false>
static void launch_step_t(MMHandle h, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
  const long long threads = (long long)h->E * G;
  const unsigned grid = kPow2<G> ? (unsigned)((threads + MM_STEP_BLOCK - 1) / MM_STEP_BLOCK)
                                 : (unsigned)((h->E + 64 / G - 1) / (64 / G));  // rotation layouts: 64 / G whole groups per wave
  if constexpr (!kFusedBuilt<KIND, MIXED, IPM>) return;
  else if (out->trace)
    hipLaunchKernelGGL((step_kernel<G, KIND, SHIELD, MIXED, IPM, true>), dim3(grid), dim3(MM_STEP_BLOCK), 0, s, dev_cfg(h), dev_state(h),
                       actions, *out, h->metrics ? h->metrics_partial : nullptr, h->sweep, 0, h->pose);
  else
    hipLaunchKernelGGL((step_kernel<G, KIND, SHIELD, MIXED, IPM, false>), dim3(grid), dim3(MM_STEP_BLOCK), 0, s, dev_cfg(h), dev_state(h),
                       actions, *out, h->metrics ? h->metrics_partial : nullptr, h->sweep, 0, h->pose);
}
// Per-env parameters (include/mm_env_params.h): the PENV instantiations of the fused kernel, shielded v1 without the trace, in
// objects of their own -- mm_penv.hip the exact-mode kernels, mm_penv_ipm.hip the interior-point ones -- for every layout
// step_group() picks, CAV-only and general.
template <int G, int SHIELD, bool MIXED, bool IPM>
static void launch_step_penv_t(MMHandle h, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
  const long long threads = (long long)h->E * G;
  const unsigned grid = kPow2<G> ? (unsigned)((threads + MM_STEP_BLOCK - 1) / MM_STEP_BLOCK)
                                 : (unsigned)((h->E + 64 / G - 1) / (64 / G));  // rotation layouts: 64 / G whole groups per wave
  if constexpr (kMixedBuilt<MIXED>)
    hipLaunchKernelGGL((step_kernel<G, MM_ENV_V1, SHIELD, MIXED, IPM, false, false, true>), dim3(grid), dim3(MM_STEP_BLOCK), 0, s, dev_cfg(h),
                       dev_state(h), actions, *out, h->metrics ? h->metrics_partial : nullptr, h->sweep, 0, h->pose);
}
template <bool IPM>
static void launch_step_penv_all(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
  const bool mass = h->cfg.shield == MM_SHIELD_MASS, general = needs_general(h);
#define MM_PENV_CASE(GG) \
  if (mass) { if (general) launch_step_penv_t<GG, MM_SHIELD_MASS, true, IPM>(h, actions, out, s); else launch_step_penv_t<GG, MM_SHIELD_MASS, false, IPM>(h, actions, out, s); } \
  else { if (general) launch_step_penv_t<GG, MM_SHIELD_HSS, true, IPM>(h, actions, out, s); else launch_step_penv_t<GG, MM_SHIELD_HSS, false, IPM>(h, actions, out, s); }
  MM_FOR_GROUP(g, MM_PENV_CASE, MM_PENV_CASE);
#undef MM_PENV_CASE
}
// The split interior-point step (SweepBuf, sweep_kernel): nsub + 1 phase launches with a sweep launch after each act half.
// All on the caller's stream: each launch reads what the previous one wrote.  (MIXED: the general kernels -- HDVs / steer_vel.)
template <int G, int SHIELD, bool MIXED>
static void launch_split_gs(MMHandle h, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
  const long long threads = (long long)h->E * G;
  const unsigned grid = kPow2<G> ? (unsigned)((threads + MM_STEP_BLOCK - 1) / MM_STEP_BLOCK)
                                 : (unsigned)((h->E + 64 / G - 1) / (64 / G));
  const DevCfg dc = dev_cfg(h);
  const DevState ds = dev_state(h);
  const unsigned sgrid = (unsigned)((h->E + 63) / 64);
  constexpr bool MASS = SHIELD == MM_SHIELD_MASS;
  for (int kb = 0; kb <= dc.nsub; kb++) {
    hipLaunchKernelGGL((step_kernel<G, MM_ENV_V1, SHIELD, MIXED, true, true, true>), dim3(grid), dim3(MM_STEP_BLOCK), 0, s, dc, ds, actions,
                       *out, h->metrics ? h->metrics_partial : nullptr, h->sweep, kb, h->pose);
    if (kb == dc.nsub) break;
    // One sweep wave per SIMD is the design point (65 536 envs = 1 024 waves = the chip's SIMDs; the kernel is bound by the
    // latency of a lone wave).  Its LDS footprint would let a CU take five single-wave workgroups -- two of them on one SIMD
    // at half speed each while another CU holds three -- so every launch asks for dynamic LDS up to 40 KB per workgroup
    // (160 KB / 4): at most four per CU.
    auto pad = [](size_t used) { return (unsigned)(used < 40960 ? 40960 - used : 0); };
    constexpr size_t kPerVeh = 6 * 64 * sizeof(double) + 3 * 64 * sizeof(unsigned short);  // s_w + s_pk / s_meta / s_cls of sweep_kernel (+ ~3 KB: verification queue)
    if (h->N <= 4) hipLaunchKernelGGL((sweep_kernel<4, MASS, MIXED>), dim3(sgrid), dim3(64), pad(4 * kPerVeh + 5632), s, dc, ds, h->sweep, kb, out->trace);
    else if (h->N <= 8) hipLaunchKernelGGL((sweep_kernel<8, MASS, MIXED>), dim3(sgrid), dim3(64), pad(8 * kPerVeh + 5632), s, dc, ds, h->sweep, kb, out->trace);
    else if (h->N <= 11) hipLaunchKernelGGL((sweep_kernel<11, MASS, MIXED>), dim3(sgrid), dim3(64), pad(11 * kPerVeh + 1024), s, dc, ds, h->sweep, kb, out->trace);  // (38 KB: density 3 = up to 11 vehicles)
    else hipLaunchKernelGGL((sweep_kernel<12, MASS, MIXED>), dim3(sgrid), dim3(64), pad(12 * kPerVeh + 1024), s, dc, ds, h->sweep, kb, out->trace);
  }
}
template <bool MIXED>
static void launch_split_all(MMHandle h, int g, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
  const bool mass = h->cfg.shield == MM_SHIELD_MASS;
#define MM_SPLIT_CASE(GG) if (mass) launch_split_gs<GG, MM_SHIELD_MASS, MIXED>(h, actions, out, s); else launch_split_gs<GG, MM_SHIELD_HSS, MIXED>(h, actions, out, s)
  if constexpr (kMixedBuilt<MIXED>) MM_FOR_GROUP(g, MM_SPLIT_CASE, MM_SPLIT_CASE);
#undef MM_SPLIT_CASE
}
template <int G, bool MIXED>
static void launch_step_m(MMHandle h, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
#ifdef MM_ONLY_SHIELD
  launch_step_t<G, MM_ENV_V1, MM_ONLY_SHIELD, MIXED>(h, actions, out, s);
  return;
#endif
  if (h->cfg.env_kind == MM_ENV_V0) { launch_step_t<G, MM_ENV_V0, MM_SHIELD_NONE, MIXED>(h, actions, out, s); return; }
  switch (h->cfg.shield) {
    case MM_SHIELD_HSS: launch_step_t<G, MM_ENV_V1, MM_SHIELD_HSS, MIXED>(h, actions, out, s); break;
    case MM_SHIELD_MASS: launch_step_t<G, MM_ENV_V1, MM_SHIELD_MASS, MIXED>(h, actions, out, s); break;
    default: launch_step_t<G, MM_ENV_V1, MM_SHIELD_NONE, MIXED>(h, actions, out, s);
  }
}
template <int G, bool MIXED>
static void launch_step_ipm_gm(MMHandle h, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
  if (h->cfg.shield == MM_SHIELD_MASS) launch_step_t<G, MM_ENV_V1, MM_SHIELD_MASS, MIXED, true>(h, actions, out, s);
  else launch_step_t<G, MM_ENV_V1, MM_SHIELD_HSS, MIXED, true>(h, actions, out, s);
}
template <int G>
static void launch_step_ipm_g(MMHandle h, const int32_t *actions, const MMStepOut *out, hipStream_t s) {
  if (needs_general(h)) launch_step_ipm_gm<G, true>(h, actions, out, s);
  else launch_step_ipm_gm<G, false>(h, actions, out, s);  // CAV-only: the lean literal-sweep kernel around the same IPM
}
