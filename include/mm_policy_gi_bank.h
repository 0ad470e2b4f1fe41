/*
 * mm_policy_gi_bank.h -- K shared actor-critics of one shape acting on the K contiguous groups of one batch, in one launch.
 *
 * The policy bank (include/mm_policy_bank.h) for MAPPO_GI with shared_network = True: every member is
 * marl/single_agent/Model_gi.py:137-216 ActorCriticNetwork(state_split=True) at hidden 128, the network of
 * include/mm_policy_gi.h, and every agent is driven (and valued) by the member of the bank that its group names.  The reference
 * trains one such model per configuration and seed and evaluates each checkpoint under its own shield setting; with per-env
 * parameters (include/mm_env_params.h) the env side of such a grid is one batch, and this entry is its policy side:
 * mm_policy_gi_act's contract with the weights chosen by the agent's group.
 *
 * Exported by libmm_hip.so only (marl-mass_amd/csrc/mm_policy_gi_bank.hip); the CPU oracle has no twin of it, and it is not
 * part of include/mm_abi.h's symbol list or version.  The CPU form is each member's torch module on its slice followed by one
 * mm_sample_actions over the whole batch (rollout.DeviceRollout's fallback).
 */
#ifndef MM_POLICY_GI_BANK_H
#define MM_POLICY_GI_BANK_H

#include <stdint.h>

#include "mm_abi.h"
#include "mm_policy_bank.h"     /* MM_BANK_MAX_GROUPS, the decomposition of a launch, mm_policy_bank_grid */
#include "mm_policy_gi_train.h" /* MMGiParams */

#ifdef __cplusplus
extern "C" {
#endif

/* K networks of one shape, stacked: `bank` holds the base pointers of DEV float W11[K][32][5], b11[K][32], W12[K][64][10],
 * b12[K][64], W13[K][64][10], b13[K][64], W2[K][128][160], b2[K][128], Wa[K][n_a][128], ba[K][n_a], Wc[K][1][128], bc[K][1]
 * (member k at base + k * size).
 * group_start: HOST int64[K + 1], group_start[0] == 0, non-decreasing, group_start[K] == n: agents
 * [group_start[k], group_start[k + 1]) are served by member k; empty groups are allowed.
 *
 * obs: DEV float[n][n_s], 25 <= n_s <= 32; hidden must be 128; 1 <= n_a <= 8; 1 <= K <= MM_BANK_MAX_GROUPS.
 * For agent i of group k:
 *   logp (optional DEV float[n][n_a]) row i and value (optional DEV float[n]) element i are, bit for bit, what mm_policy_gi_act
 *     writes for that observation with member k's weights -- a row's arithmetic depends neither on the lane or tile it sits in,
 *     nor on its group's offset, nor on how the grid is split (mm_policy_bank_grid's split, MM_BANK_* of mm_policy_bank.h).
 *   actions (DEV int32[n], or NULL): the draw mm_sample_actions makes from that row with key (seed, *counter, i), i the GLOBAL
 *     agent index.  Non-NULL: *counter (DEV) is read by the launch and incremented by one on the stream after it.  NULL: nothing
 *     is sampled and counter is neither read nor written (it may be NULL).
 * At least one of actions / logp / value must be given.
 * Only enqueues work on `stream`: graph-capturable.  group_start is copied into the kernel's by-value argument block when the
 * launch is enqueued: the caller's host array is not read afterwards.
 * n = 0: MM_OK, nothing is enqueued and *counter stays as it is.
 * Observations must be finite in the columns the split reads, as for mm_policy_gi_act.
 * MM_ERR_INVALID_ARG, before anything is enqueued: NULL obs, bank or group_start, a NULL member base, K outside
 *   1..MM_BANK_MAX_GROUPS, hidden != 128, n_s outside 25..32, n_a outside 1..8, n < 0, no output, actions without counter, a
 *   group_start that does not start at 0, decreases or does not end at n.
 */
int32_t mm_policy_gi_bank_act(const float *obs, int64_t n, int32_t n_s, const MMGiParams *bank, int32_t K,
                              const int64_t *group_start, int32_t hidden, int32_t n_a, uint64_t seed, uint64_t *counter,
                              int32_t *actions, float *logp, float *value, MMStream stream);

#ifdef __cplusplus
}
#endif
#endif /* MM_POLICY_GI_BANK_H */
