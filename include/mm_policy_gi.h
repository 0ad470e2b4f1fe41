/*
 * mm_policy_gi.h -- the shared actor-critic of MAPPO_GI (shared_network = True) as one launch.
 *
 * marl/single_agent/Model_gi.py:137-216 ActorCriticNetwork(state_split=True), hidden 128:
 *   state1 = state[:, 0::5][:5]          (columns 0, 5, 10, 15, 20)          -> fc11  5 -> 32,  ReLU
 *   state2 = state[:, 1:3, 6:8, .., 21:23] (columns 1-2 of each 5-column block) -> fc12 10 -> 64,  ReLU
 *   state3 = state[:, 3:5, 8:10, .., 23:25] (columns 3-4 of each block)        -> fc13 10 -> 64,  ReLU
 *   out = relu(fc2(cat(out1, out2, out3)))                                     160 -> 128
 *   logp = log_softmax(actor_linear(out))   (out_type "p", no action mask)     128 -> n_a
 *   value = critic_linear(out)              (out_type "v")                     128 -> 1
 * followed by the categorical sample of MAPPO_GI.exploration_action / action (marl/mappo_gi.py:355-377).
 * The split reads columns 0..24 as if every observation row had 5 columns, whatever n_s is: on merge-multi-agent-v1
 * (KinematicLC, 6 columns per row, n_s = 30) columns 25..29 are never read.  That is the reference's behaviour, kept.
 *
 * Exported by libmm_hip.so only (marl-mass_amd/csrc/mm_policy_gi.hip); the CPU oracle has no twin of it, and it is not
 * part of include/mm_abi.h's symbol list or version.  The torch module rollout.ActorCriticNetwork is the CPU form.
 */
#ifndef MM_POLICY_GI_H
#define MM_POLICY_GI_H

#include <stdint.h>

#include "mm_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * obs: DEV float[n][n_s], 25 <= n_s <= 32.  Weights in torch nn.Linear layout [out][in], float32, DEV:
 *   W11 [32][5],  b11 [32];  W12 [64][10], b12 [64];  W13 [64][10], b13 [64];  W2 [128][160], b2 [128];
 *   Wa [n_a][128], ba [n_a];  Wc [1][128], bc [1].
 * hidden must be 128 (the reference's only value); 1 <= n_a <= 8.
 * actions: DEV int32[n], or NULL.  Non-NULL: every agent draws its action exactly as mm_sample_actions /
 *   mm_policy_act do (Philox4x32-10 keyed on the agent index, *counter and the same domain word; fp64 inverse CDF), and
 *   *counter is incremented by one on the stream after the launch.  NULL: value-only mode, nothing is sampled and
 *   counter is neither read nor written (it may be NULL).
 * logp: optional DEV float[n][n_a] (the log-softmax the sample is drawn from); value: optional DEV float[n].
 * At least one of actions / logp / value must be given.  Only enqueues work on `stream`: graph-capturable.
 * n = 0: MM_OK, nothing is enqueued and *counter stays as it is.
 * Observations must be finite in the columns the split reads (0..24; columns 25..n_s-1 are never read).  Non-finite
 *   observations are outside the contract: fmaxf drops a NaN pre-activation where torch's relu keeps it.  (A non-finite row
 *   still reaches no other row's outputs.)
 * MM_ERR_INVALID_ARG: NULL weights, n < 0, n_s outside 25..32, hidden != 128, n_a outside 1..8, no output,
 *   actions without counter.
 */
int32_t mm_policy_gi_act(const float *obs, int64_t n, int32_t n_s, const float *W11, const float *b11, const float *W12,
                         const float *b12, const float *W13, const float *b13, const float *W2, const float *b2,
                         const float *Wa, const float *ba, const float *Wc, const float *bc, int32_t hidden, int32_t n_a,
                         uint64_t seed, uint64_t *counter, int32_t *actions, float *logp, float *value, MMStream stream);

#ifdef __cplusplus
}
#endif
#endif /* MM_POLICY_GI_H */
