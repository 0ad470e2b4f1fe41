/*
 * mm_policy_bank_train.h -- the training half of the policy bank (include/mm_policy_bank.h is the acting half): K actor / critic
 * pairs of one shape, each trained on its own contiguous column group of ONE batch, in launch sets whose size depends neither
 * on K nor on the group sizes.
 *
 * Every member is MAPPO's separate actor and critic at hidden 128 (include/mm_policy_train.h: the networks, the objective, the
 * two forms of the actor loss).  What the three entries compute for member k is, bit for bit, what mm_policy_eval /
 * mm_policy_train compute on member k's samples gathered in member-local order with member k's parameters; what is new is that
 * all members run in the same launches (the optimiser tail is mm_opt_step_bank, include/mm_opt_step.h).
 *
 * Parameters and gradients are STACKED MMMlpParams, as in mm_policy_bank.h: member k at base + k * tensor size,
 *   actor:  W1 [K][128][n_s], b1 [K][128]; W2 [K][128][128],       b2 [K][128]; W3 [K][n_a][128], b3 [K][n_a]
 *   critic: W1 [K][128][n_s], b1 [K][128]; W2 [K][128][128 + n_a], b2 [K][128]; W3 [K][1][128],   b3 [K][1]
 *
 * Sample addressing (all entries).  A batch is `rows` rows of `row_len` samples, n = rows * row_len <= 2^31 - 1.  Sample
 * j = r * row_len + c lives at obs + j * obs_stride, actions[j * act_stride], returns[j * ret_stride]; the per-sample [n] arrays
 * (old_logp, valid, advantages, target_value, the diagnostics) are indexed by the same j.  col_start: HOST int64[K + 1],
 * col_start[0] == 0, non-decreasing, col_start[K] == row_len: member k owns columns [col_start[k], col_start[k + 1]) of every
 * row, w_k of them, n_k = rows * w_k samples; its samples in member-local order are i = r * w_k + (c - col_start[k]).  Empty
 * groups are allowed; 1 <= K <= MM_BANK_MAX_GROUPS.  col_start is copied into the kernels' by-value argument blocks when the
 * launches are enqueued: the host array is not read afterwards, and every entry is graph-capturable.
 * This addresses DeviceRollout.interact()'s [T, E, N, S] batch in place: reference form, agent a: rows = T, row_len = E, base
 * pointers offset by a (obs: a * S), obs_stride = N * S, act_stride = ret_stride = N, col_start = the env prefix; flat form:
 * rows = T, row_len = E * N, obs_stride = S, col_start = the env prefix times N.
 *
 * Exported by libmm_hip.so only (marl-mass_amd/csrc/mm_policy_bank_train.hip); no oracle twin, not part of include/mm_abi.h's
 * symbol list or version.  Shared actor-critic members are include/mm_policy_gi_bank_train.h's.  Out of scope: hidden 512, the
 * chunked and rank-sharded forms, per-member hyperparameters.
 */
#ifndef MM_POLICY_BANK_TRAIN_H
#define MM_POLICY_BANK_TRAIN_H

#include <stdint.h>

#include "mm_abi.h"
#include "mm_policy_bank.h"  /* MM_BANK_MAX_GROUPS */
#include "mm_policy_train.h" /* MMMlpParams, MM_PT_CRITIC_* */

#ifdef __cplusplus
extern "C" {
#endif

#define MM_PT_FORM_REFERENCE 0  /* the reference's [B, B] objective, S+_k / S-_k summed over group k */
#define MM_PT_FORM_PER_SAMPLE 1 /* textbook per-sample PPO-clip */

/*
 * Forward only: logp_taken[j] from member k's actor, value[j] from member k's critic, k the group sample j falls in.
 * actors with logp_taken, critics with value: either pair may be NULL (both pointers of the pair), not both pairs.  Masked
 * slots (valid[j] == 0) are not read and get 0.  n == 0 does nothing.  Two launches at most (one per given network).
 * MM_ERR_INVALID_ARG, before anything is enqueued: no network, a network without its output or the reverse, a NULL base among a
 *   given network's six, obs / actions / col_start NULL, rows or row_len < 0, n > 2^31 - 1, n_s outside 25..32, obs_stride < n_s,
 *   hidden != 128, n_a outside 1..8, K outside 1..MM_BANK_MAX_GROUPS, a col_start that does not start at 0, decreases or does
 *   not end at row_len.
 */
int32_t mm_policy_bank_eval(const float *obs, int64_t obs_stride, int64_t rows, int64_t row_len, int32_t n_s, const int32_t *actions,
                            int64_t act_stride, const uint8_t *valid, const MMMlpParams *actors, const MMMlpParams *critics,
                            int32_t K, const int64_t *col_start, int32_t hidden, int32_t n_a, float *logp_taken, float *value,
                            MMStream stream);

/*
 * Bytes of scratch mm_policy_bank_train needs: MM_PBT_HEADER_BYTES, K times MM_PBT_MEMBER_BYTES (both networks' transposed fc2
 * fragments), and for every group of n_k = rows * w_k samples, t_k = ceil(n_k / 32) tiles:
 *   32 t_k * MM_PBT_SAMPLE_BYTES   the per-sample rows of kernel A (one network at a time, as mm_policy_train)
 *   t_k * MM_PBT_TILE_BYTES        fp64 per tile: one loss partial and the three statistics (B_k, S+_k, S-_k)
 *   min(ceil(t_k / 2), 512) * MM_PBT_PARTIAL_BYTES   room for kernel B's partial blocks.  (The group's own decomposition,
 *     mm_policy_train's on n_k samples, uses ceil(t_k / max(2, ceil(t_k / 512))) of them; the bound is what makes the query
 *     non-decreasing in every width.)
 * MM_ERR_INVALID_ARG: bytes NULL, rows < 0, n > 2^31 - 1, K or col_start as above (col_start[K] is row_len).
 */
#define MM_PBT_HEADER_BYTES 1024
#define MM_PBT_MEMBER_BYTES 131072
#define MM_PBT_SAMPLE_BYTES 2240
#define MM_PBT_TILE_BYTES 32
#define MM_PBT_PARTIAL_BYTES 107584
int32_t mm_policy_bank_train_scratch_bytes(int64_t rows, int64_t row_len, int32_t K, const int64_t *col_start, uint64_t *bytes);

/*
 * mm_policy_train's objective, separately for every member: B_k is the number of valid samples of group k.
 * Inputs as mm_policy_train's (addressed as above), and
 *   form        MM_PT_FORM_REFERENCE or MM_PT_FORM_PER_SAMPLE.
 *   advantages / target_value   with actors exactly one of them, DEV float[n]: the per-sample advantage, given directly or as
 *               returns_j - target_value_j in float32 (one rounding; target_value is the critic target's output from
 *               mm_policy_bank_eval), 0 where masked.  In the reference form S+_k / S-_k (the sums of the non-negative /
 *               negative advantages of group k's valid samples) are accumulated in fp64 in a fixed order (a butterfly per
 *               32-sample tile, then a fixed tree over the group's tiles) and rounded once to float.
 * Outputs: actor_grads / critic_grads, stacked, WRITTEN (not accumulated); loss DEV float[K][2] (actor, critic; 0 for an
 *   omitted network); adv_sums optional DEV float[K][2]: the S+_k, S-_k that were used (zeros in the per-sample form and without
 *   actors); logp_taken / value / ratio optional DEV float[n] diagnostics, 0 where masked.
 * A group that is empty or has no valid sample gets zero gradients and zero losses.
 * No floating-point atomics anywhere: two calls on equal inputs give equal bits.  Only enqueues on `stream`; a refused call
 * enqueues nothing.
 *
 * The defining property: member k's gradients, losses and diagnostics are bit for bit those of mm_policy_train on member k's
 * samples gathered in member-local order with member k's parameters, given the same adv_sums (reference form) or the same
 * advantages (per-sample form).  They depend on no other member's samples or parameters and on no other group's size or
 * position: each group keeps mm_policy_train's decomposition of n_k samples -- tiles counted from the group's own start,
 * kernel-B slices of whole tiles of one group, the loss tree over the group's own tiles.
 *
 * The launches, whatever K is: the fragments of all members; the statistics per tile and their fold per group; then per given
 * network kernel A (a workgroup serves one group: it stages that member's fragments once and walks that group's tiles; the grid
 * is mm_policy_bank_grid's split), kernel B (grid = the sum of the groups' slices) and kernel C (grid x K).
 *
 * MM_ERR_INVALID_ARG: as mm_policy_bank_eval for the shared arguments, and: no network, a network without gradients or the
 *   reverse, loss NULL, critic_loss or form not one of the two, clip_param < 0, a diagnostic of an omitted network, and with
 *   n > 0 (with n == 0 the per-sample inputs and the scratch are not looked at and may be NULL): with actors both or neither of
 *   advantages / target_value, old_logp NULL with actors, returns NULL with critics or with target_value, scratch NULL /
 *   misaligned (16 bytes) / smaller than the query.
 */
int32_t mm_policy_bank_train(const float *obs, int64_t obs_stride, int64_t rows, int64_t row_len, int32_t n_s, const int32_t *actions,
                             int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp, const uint8_t *valid,
                             const MMMlpParams *actors, const MMMlpParams *critics, int32_t K, const int64_t *col_start,
                             int32_t hidden, int32_t n_a, float clip_param, int32_t critic_loss, int32_t form,
                             const float *advantages, const float *target_value, const MMMlpParams *actor_grads,
                             const MMMlpParams *critic_grads, float *loss, float *adv_sums, float *logp_taken, float *value,
                             float *ratio, void *scratch, uint64_t scratch_bytes, MMStream stream);

#ifdef __cplusplus
}
#endif
#endif /* MM_POLICY_BANK_TRAIN_H */
