/*
 * mm_policy_bank.h -- K actors of one shape acting on the K contiguous groups of one batch, in one launch.
 *
 * The reference trains one model per configuration (per cbf_eta, per shield, per reward variant, three seeds each) and
 * evaluates each checkpoint under its own setting (run_mappo.py evaluate, eta_binary_search.sh).  With per-env parameters
 * (include/mm_env_params.h) the env side of such a grid is one batch; this entry is the policy side: every agent is driven by
 * the member of the bank that its group names.  Each member is marl/single_agent/Model_common.py:5-22 ActorNetwork at hidden
 * 128 (n_s -> 128 -> 128 -> n_a, ReLU, log-softmax), followed by the categorical sample of MAPPO.exploration_action / action
 * (marl/mappo.py:220-236): mm_policy_act's contract (include/mm_abi.h), with the weights chosen by the agent's group.
 *
 * Exported by libmm_hip.so only (marl-mass_amd/csrc/mm_policy_bank.hip); the CPU oracle has no twin of it, and it is not
 * part of include/mm_abi.h's symbol list or version.  The CPU form is each member's torch module on its slice followed by one
 * mm_sample_actions over the whole batch (rollout.DeviceRollout's fallback).
 */
#ifndef MM_POLICY_BANK_H
#define MM_POLICY_BANK_H

#include <stdint.h>

#include "mm_abi.h"
#include "mm_policy_train.h" /* MMMlpParams */

#ifdef __cplusplus
extern "C" {
#endif

#define MM_BANK_MAX_GROUPS 64
/* The decomposition of a launch, for callers that test its boundaries: a wave owns one tile of MM_BANK_TILE agents at a time,
 * counted from its group's own start; a workgroup has MM_BANK_WAVES waves and serves one group; the grid is split over the
 * non-empty groups in proportion to their tiles, at least one workgroup each, at most MM_BANK_MAX_GRID + K in all.  A row's
 * outputs depend on none of them. */
#define MM_BANK_TILE 32
#define MM_BANK_WAVES 8
#define MM_BANK_MAX_GRID 256

/* K actors of one shape (Model_common.py ActorNetwork, n_s -> 128 -> 128 -> n_a), stacked: `bank` holds the base pointers of
 * DEV float W1[K][128][n_s], b1[K][128], W2[K][128][128], b2[K][128], W3[K][n_a][128], b3[K][n_a] (member k at base + k * size).
 * group_start: HOST int64[K + 1], group_start[0] == 0, non-decreasing, group_start[K] == n: agents
 * [group_start[k], group_start[k + 1]) are served by member k; empty groups are allowed.
 *
 * obs: DEV float[n][n_s], 1 <= n_s <= 32; hidden must be 128; 1 <= n_a <= 8; 1 <= K <= MM_BANK_MAX_GROUPS.
 * For agent i of group k:
 *   logp (optional DEV float[n][n_a]): row i is, bit for bit, the row mm_policy_act writes for that observation with member
 *     k's weights -- a row's arithmetic depends neither on the lane or tile it sits in nor on how the grid is split.
 *   actions (DEV int32[n]): the draw mm_sample_actions makes from that row with key (seed, *counter, i), i the GLOBAL agent
 *     index (Philox4x32-10, domain word 0x53414D50; fp64 inverse CDF).
 * *counter (DEV) is read by the launch and incremented by one on the stream after it.
 * Only enqueues work on `stream`: graph-capturable.  group_start is copied into the kernel's by-value argument block when the
 * launch is enqueued: the caller's host array is not read afterwards.
 * n = 0: MM_OK, nothing is enqueued and *counter stays as it is.
 * Observations must be finite, as for mm_policy_act.
 * MM_ERR_INVALID_ARG, before anything is enqueued: a NULL pointer other than logp or a NULL member base, K outside
 *   1..MM_BANK_MAX_GROUPS, hidden != 128, n_s outside 1..32, n_a outside 1..8, n < 0, a group_start that does not start at 0,
 *   decreases or does not end at n.
 */
int32_t mm_policy_bank_act(const float *obs, int64_t n, int32_t n_s, const MMMlpParams *bank, int32_t K,
                           const int64_t *group_start, int32_t hidden, int32_t n_a, uint64_t seed, uint64_t *counter,
                           int32_t *actions, float *logp, MMStream stream);

/* The grid split of such a launch, computed on the host alone (no device is touched): block_start (HOST int32[K + 1]) receives
 * the prefix of the workgroups per group -- group k is served by workgroups [block_start[k], block_start[k + 1]), none for an
 * empty group, block_start[K] the grid.  MM_ERR_INVALID_ARG for a NULL pointer, K outside 1..MM_BANK_MAX_GROUPS or a
 * group_start that does not start at 0 or decreases. */
int32_t mm_policy_bank_grid(int32_t K, const int64_t *group_start, int32_t *block_start);

#ifdef __cplusplus
}
#endif
#endif /* MM_POLICY_BANK_H */
