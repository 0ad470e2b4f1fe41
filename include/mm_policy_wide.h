/*
 * mm_policy_wide.h -- the reference's hidden-512 actor (lateral_control = steer_vel configurations) as one launch.
 *
 * marl/single_agent/Model_common.py:5-22 ActorNetwork with actor_hidden_size = 512: n_s -> 512 -> 512 -> n_a, ReLU,
 * log-softmax, followed by the categorical sample of MAPPO.exploration_action / action (marl/mappo.py:220-236).
 * It is mm_policy_act's contract (include/mm_abi.h) at the other hidden size the reference trains with, and
 * mm_policy_act(..., hidden = 512, ...) forwards here.
 *
 * Exported by libmm_hip.so only (marl-mass_amd/csrc/mm_policy_wide.hip); the CPU oracle has no twin of it, and it is not
 * part of include/mm_abi.h's symbol list or version.  The torch module rollout.ActorNetwork is the CPU form.
 */
#ifndef MM_POLICY_WIDE_H
#define MM_POLICY_WIDE_H

#include <stdint.h>

#include "mm_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The decomposition of a launch, for callers that test its boundaries: a wave owns one tile of MM_POLICY_WIDE_TILE agents at
 * a time, a workgroup has MM_POLICY_WIDE_WAVES waves, and at most MM_POLICY_WIDE_MAX_GRID persistent workgroups are launched
 * (each walks tile groups blockIdx, blockIdx + grid, ...).  A row's outputs depend on none of them. */
#define MM_POLICY_WIDE_TILE 32
#define MM_POLICY_WIDE_WAVES 4
#define MM_POLICY_WIDE_MAX_GRID 256
/* fc2's weight is read with 16-byte loads: W2 must be aligned to this many bytes (a torch allocation is; a view that starts
 * 4 bytes into one is not).  No other pointer needs more than its element's alignment. */
#define MM_POLICY_WIDE_W2_ALIGN 16

/*
 * obs: DEV float[n][n_s], 1 <= n_s <= 32.  Weights in torch nn.Linear layout [out][in], float32, DEV:
 *   W1 [512][n_s], b1 [512];  W2 [512][512], b2 [512];  W3 [n_a][512], b3 [n_a].
 * hidden must be 512; 1 <= n_a <= 8.  W2 must be MM_POLICY_WIDE_W2_ALIGN-byte aligned.
 * actions: DEV int32[n].  Every agent draws its action exactly as mm_sample_actions does on this call's own logp
 *   (Philox4x32-10 keyed on the agent index, *counter and the domain word 0x53414D50; fp64 inverse CDF), and *counter is
 *   incremented by one on the stream after the launch.
 * logp: optional DEV float[n][n_a], the log-softmax the sample is drawn from:
 *   logp = (logit - max) - log(sum exp(logit - max)), torch's order.
 * Only enqueues work on `stream`: graph-capturable.  n = 0: MM_OK, nothing is enqueued and *counter stays as it is.
 * Observations must be finite.  Non-finite observations are outside the contract: fmaxf drops a NaN pre-activation where
 *   torch's relu keeps it.  (A non-finite row still reaches no other row's outputs.)
 * A row's outputs are a function of that row and the weights alone: not of n, nor of where the row falls in the launch.
 * MM_ERR_INVALID_ARG: a NULL pointer other than logp, n < 0, n_s outside 1..32, hidden != 512, n_a outside 1..8, W2 off its
 *   alignment (an argument check: nothing is launched).
 */
int32_t mm_policy_wide_act(const float *obs, int64_t n, int32_t n_s, const float *W1, const float *b1, const float *W2,
                           const float *b2, const float *W3, const float *b3, int32_t hidden, int32_t n_a, uint64_t seed,
                           uint64_t *counter, int32_t *actions, float *logp, MMStream stream);

#ifdef __cplusplus
}
#endif
#endif /* MM_POLICY_WIDE_H */
