/*
 * mm_policy_gi_bank_train.h -- the training half of the bank of shared actor-critics (include/mm_policy_gi_bank.h is the acting
 * half): K networks of one shape, each trained on its own contiguous column group of ONE batch, in a launch set whose size
 * depends neither on K nor on the group sizes.
 *
 * Every member is MAPPO_GI's shared network at hidden 128 (include/mm_policy_gi_train.h: the network, the objective, the two
 * forms of the actor loss).  What the entries compute for member k is, bit for bit, what mm_policy_gi_act / mm_policy_gi_train
 * compute on member k's samples gathered in member-local order with member k's parameters; what is new is that all members run
 * in the same launches (the optimiser tail is mm_opt_step_bank, include/mm_opt_step.h: the twelve tensors are one prototype
 * group).
 *
 * Parameters and gradients are STACKED MMGiParams, as in mm_policy_gi_bank.h: member k at base + k * tensor size,
 *   W11 [K][32][5], b11 [K][32], W12 [K][64][10], b12 [K][64], W13 [K][64][10], b13 [K][64], W2 [K][128][160], b2 [K][128],
 *   Wa [K][n_a][128], ba [K][n_a], Wc [K][1][128], bc [K][1].
 *
 * Sample addressing is mm_policy_bank_train.h's, word for word.  A batch is `rows` rows of `row_len` samples,
 * n = rows * row_len <= 2^31 - 1.  Sample j = r * row_len + c lives at obs + j * obs_stride, actions[j * act_stride],
 * returns[j * ret_stride]; the per-sample [n] arrays (old_logp, valid, value_now, the diagnostics) are indexed by the same j.
 * col_start: HOST int64[K + 1], col_start[0] == 0, non-decreasing, col_start[K] == row_len: member k owns columns
 * [col_start[k], col_start[k + 1]) of every row, w_k of them, n_k = rows * w_k samples; its samples in member-local order are
 * i = r * w_k + (c - col_start[k]).  Empty groups are allowed; 1 <= K <= MM_BANK_MAX_GROUPS.  col_start is copied into the
 * kernels' by-value argument blocks when the launches are enqueued: the host array is not read afterwards, and every entry is
 * graph-capturable.
 * This addresses DeviceRollout.interact()'s [T, E, N, S] batch in place: reference form, agent a: rows = T, row_len = E, base
 * pointers offset by a (obs: a * S), obs_stride = N * S, act_stride = ret_stride = N, col_start = the env prefix; flat form:
 * rows = T, row_len = E * N, obs_stride = S, col_start = the env prefix times N.
 *
 * Exported by libmm_hip.so only (marl-mass_amd/csrc/mm_policy_gi_bank_train.hip); no oracle twin, not part of include/mm_abi.h's
 * symbol list or version.  Out of scope: hidden 512, the chunked and rank-sharded forms, per-member hyperparameters.
 */
#ifndef MM_POLICY_GI_BANK_TRAIN_H
#define MM_POLICY_GI_BANK_TRAIN_H

#include <stdint.h>

#include "mm_abi.h"
#include "mm_policy_bank.h"       /* MM_BANK_MAX_GROUPS */
#include "mm_policy_bank_train.h" /* MM_PT_FORM_* */
#include "mm_policy_gi_train.h"   /* MMGiParams, MM_GI_CRITIC_* */

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Forward only, one launch: for sample j of group k, logp_taken[j] and value[j] (DEV float[n], at least one of them) are, bit
 * for bit, what mm_policy_gi_act writes for that observation with member k's weights: the log-probability row's entry at
 * clamp(actions[j], 0, n_a - 1), and the value.  Masked slots (valid[j] == 0) are not read and get 0.  n == 0 does nothing, and
 * the per-sample pointers (obs, actions, the outputs) are not looked at.
 * MM_ERR_INVALID_ARG, before anything is enqueued: no output, bank NULL or a NULL base among its twelve, obs / actions /
 *   col_start NULL, rows or row_len < 0, n > 2^31 - 1, n_s outside 25..32, obs_stride < n_s, hidden != 128, n_a outside 1..8,
 *   K outside 1..MM_BANK_MAX_GROUPS, a col_start that does not start at 0, decreases or does not end at row_len.
 */
int32_t mm_policy_gi_bank_eval(const float *obs, int64_t obs_stride, int64_t rows, int64_t row_len, int32_t n_s, const int32_t *actions,
                               int64_t act_stride, const uint8_t *valid, const MMGiParams *bank, int32_t K, const int64_t *col_start,
                               int32_t hidden, int32_t n_a, float *logp_taken, float *value, MMStream stream);

/*
 * Bytes of scratch mm_policy_gi_bank_train needs: MM_GBT_HEADER_BYTES, K times MM_GBT_MEMBER_BYTES (the 5 * 4 * 4 * 64 float4
 * fragments of one W2^T), and for every group of n_k = rows * w_k samples, t_k = ceil(n_k / 32) tiles:
 *   32 t_k * MM_GBT_SAMPLE_BYTES   the per-sample rows of kernel A: h1, dz1 of 160 floats, h2, dz2 of 128, 16 and 32 floats
 *   t_k * MM_GBT_TILE_BYTES        fp64 per tile: the two loss partials and the three statistics (B_k, S+_k, S-_k)
 *   min(ceil(t_k / 2), 512) * MM_GBT_PARTIAL_BYTES   room for kernel B's partial blocks.  (The group's own decomposition,
 *     mm_policy_gi_train's on n_k samples, uses ceil(t_k / max(2, ceil(t_k / 512))) of them; the bound is what makes the query
 *     non-decreasing in every width.)
 * MM_ERR_INVALID_ARG: bytes NULL, rows < 0, n > 2^31 - 1, K or col_start as above (col_start[K] is row_len).
 */
#define MM_GBT_HEADER_BYTES 1024
#define MM_GBT_MEMBER_BYTES 81920
#define MM_GBT_SAMPLE_BYTES 2496
#define MM_GBT_TILE_BYTES 40
#define MM_GBT_PARTIAL_BYTES 111808
int32_t mm_policy_gi_bank_train_scratch_bytes(int64_t rows, int64_t row_len, int32_t K, const int64_t *col_start, uint64_t *bytes);

/*
 * mm_policy_gi_train's objective, separately for every member: B_k is the number of valid samples of group k.
 * Inputs as mm_policy_gi_train's (addressed as above), and
 *   form        MM_PT_FORM_REFERENCE or MM_PT_FORM_PER_SAMPLE (include/mm_policy_bank_train.h).
 *   value_now   reference form: required, DEV float[n], the live members' value from mm_policy_gi_bank_eval.  The per-sample
 *               advantage is returns_j - value_now_j in float32 (one rounding); S+_k / S-_k (the sums of the non-negative /
 *               negative advantages of group k's valid samples) are accumulated in fp64 in a fixed order (a butterfly per
 *               32-sample tile, then a fixed tree over the group's tiles) and rounded once to float.
 *               per-sample form: must be NULL; A_j = returns_j - value_j comes from the launch's own forward, as in
 *               mm_policy_gi_train with adv_sums == NULL.
 * Outputs: grads, stacked, WRITTEN (not accumulated); loss DEV float[K][3] (actor, critic, their sum); adv_sums optional DEV
 *   float[K][2]: the S+_k, S-_k that were used (zeros in the per-sample form); logp_taken / value / ratio optional DEV float[n]
 *   diagnostics, 0 where masked.
 * A group that is empty or has no valid sample gets zero gradients and zero losses.
 * No floating-point atomics anywhere: two calls on equal inputs give equal bits.  Only enqueues on `stream`; a refused call
 * enqueues nothing.
 *
 * The defining property: member k's gradients, losses and diagnostics are bit for bit those of mm_policy_gi_train on member k's
 * samples gathered in member-local order with member k's parameters, given (reference form) the same adv_sums.  They depend on
 * no other member's samples or parameters and on no other group's size or position: each group keeps mm_policy_gi_train's
 * decomposition of n_k samples -- tiles counted from the group's own start, kernel-B slices of whole tiles of one group, the
 * loss tree over the group's own tiles.
 *
 * Six launches, whatever K is: the W2^T fragments of all members; the statistics per tile and their fold per group; kernel A
 * (a workgroup serves one group: it stages that member's weights once and walks that group's tiles; MM_BANK_WAVES waves, the
 * grid is mm_policy_bank_grid's split); kernel B (grid = the sum of the groups' slices); kernel C (grid x K).
 *
 * MM_ERR_INVALID_ARG: as mm_policy_gi_bank_eval for the shared arguments, and: grads NULL or incomplete, loss NULL,
 *   critic_loss or form not one of the two, clip_param < 0, and with n > 0 (with n == 0 the per-sample inputs and the scratch
 *   are not looked at and may be NULL): returns or old_logp NULL, value_now NULL in the reference form or given in the
 *   per-sample form, scratch NULL / misaligned (16 bytes) / smaller than the query.
 */
int32_t mm_policy_gi_bank_train(const float *obs, int64_t obs_stride, int64_t rows, int64_t row_len, int32_t n_s,
                                const int32_t *actions, int64_t act_stride, const float *returns, int64_t ret_stride,
                                const float *old_logp, const uint8_t *valid, const MMGiParams *bank, int32_t K,
                                const int64_t *col_start, int32_t hidden, int32_t n_a, float clip_param, int32_t critic_loss,
                                int32_t form, const float *value_now, const MMGiParams *grads, float *loss, float *adv_sums,
                                float *logp_taken, float *value, float *ratio, void *scratch, uint64_t scratch_bytes,
                                MMStream stream);

#ifdef __cplusplus
}
#endif
#endif /* MM_POLICY_GI_BANK_TRAIN_H */
