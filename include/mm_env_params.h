/*
 * mm_env_params.h -- per-env shield parameters: every env of a batch with its own cbf_eta, cbf_tau and HEADWAY_TIME.
 *
 * The reference keeps the shield's two tuning knobs as class globals (CBFType.GAMMA_B = eta, CBFType.TAU, set once per
 * process by run_mappo.py:138-139) and tunes them by running the whole program once per value
 * (test/cbf/eta_binary_search.sh; the .ini files differ in HEADWAY_TIME).  Here the three numbers are planes over the
 * batch's envs, read by the step kernel where it would read the MMConfig values, so one launch steps a whole
 * eta x tau x HEADWAY_TIME grid (x seeds) and a training batch can randomise the safety margin per env.
 *
 * Exported by libmm_hip.so only (marl-mass_amd/csrc/mm_main.hip); the CPU oracle has no counterpart, its envs are
 * uniform.  Optional symbol, like mm_supervise_dmc: MM_ABI_VERSION does not change and a caller looks it up before use.
 *
 * Scope: merge-multi-agent-v1 with the HSS or MASS shield (cbf-avs_cint / cbf-cav), both QP modes, CAV-only and mixed
 * traffic, steer_vel.  While the planes are set
 *   - mm_step runs the fused per-env instantiations of the step kernel; a batch that would otherwise take the split
 *     interior-point step (phase + sweep launches) runs the fused kernel instead: the same results, slower at large E;
 *   - mm_step with MMStepOut.trace != NULL and mm_shield_actions return MM_ERR_INVALID_ARG (neither has a per-env
 *     form; they do not fall back to the uniform values);
 *   - mm_set_config keeps them, and refuses a configuration outside the scope above.
 * mm_reset, mm_observe, mm_init_from_kinematics, the metrics and the auto-reset read none of the three values.
 */
#ifndef MM_ENV_PARAMS_H
#define MM_ENV_PARAMS_H

#include <stdint.h>

#include "mm_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MM_ENVP_ETA = 0, MM_ENVP_TAU = 1, MM_ENVP_HEADWAY_TIME = 2, MM_ENVP_COUNT = 3 };

/*
 * params: DEV double[MM_ENVP_COUNT][E] (plane p of env e at params[p * E + e]), caller-owned and alive for as long as it
 *         is set, or NULL = off: the handle's MMConfig values again.
 * Every mm_step after the call reads the planes when it runs; their contents may change between steps (stream-ordered),
 * so a captured rollout graph sees updates.  The values are not validated on the device: the caller keeps them finite and
 * cbf_tau, HEADWAY_TIME positive.  A batch whose planes hold the MMConfig values steps to the bits of the uniform kernels.
 * MM_ERR_INVALID_ARG (reason in mm_last_error): a handle that is not MM_ENV_V1 with MM_SHIELD_HSS or MM_SHIELD_MASS.
 */
int32_t mm_set_env_params(MMHandle h, const double *params);

#ifdef __cplusplus
}
#endif
#endif /* MM_ENV_PARAMS_H */
