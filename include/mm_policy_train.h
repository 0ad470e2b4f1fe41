/*
 * mm_policy_train.h -- loss and full parameter gradient of MAPPO's separate actor and critic (shared_network = False).
 *
 * The networks are Model_common.py:5-41 (rollout.ActorNetwork / rollout.CriticNetwork), hidden 128:
 *   actor    fc1 n_s -> 128, ReLU; fc2 128 -> 128, ReLU; fc3 128 -> n_a, log-softmax
 *   critic   fc1 n_s -> 128, ReLU; fc2 (128 + n_a) -> 128 on cat([h1, one_hot(action)]), ReLU; fc3 128 -> 1
 * and the objective is one agent step of MAPPO.train() (marl/mappo.py:170-201) for ONE batch of samples:
 *
 *   logp_j  = actor(obs_j)[action_j]                                    value_j = critic(obs_j, one_hot(action_j))
 *   r_j     = exp(logp_j - old_logp_j)                                  c_j = clip(r_j, 1 - clip_param, 1 + clip_param)
 *   critic  = (1 / B) sum_j l(value_j - returns_j)       l(d) = d^2 (MM_PT_CRITIC_MSE) | smooth_l1, beta = 1 (MM_PT_CRITIC_HUBER)
 *   actor   = one of two forms:
 *     adv_sums != NULL     the reference's own arithmetic.  There `ratio` is [B] and `advantages = returns - critic_target(s, a)`
 *                          is [B, 1], so `ratio * advantages` broadcasts to [B, B] and the loss is
 *                          -mean_{i,j} min(r_j A_i, c_j A_i) = -(1 / B^2) sum_j [S+ min(r_j, c_j) + S- max(r_j, c_j)],
 *                          S+ = sum of the non-negative A_i, S- = sum of the negative A_i: adv_sums = DEV float[2] {S+, S-}.
 *     advantages != NULL   textbook PPO-clip, -(1 / B) sum_j min(r_j A_j, c_j A_j), A_j = advantages[j] (DEV float[n]).
 *   In both forms the advantages are an INPUT: in MAPPO they come from another network (the critic target, through
 *   mm_policy_eval), not from the critic being trained.
 * The two losses read disjoint parameters, so both gradients are taken from the pre-step parameters in one call.
 * B is the number of valid samples (valid == NULL: n).  d min(r, c)/dr is 1 for r <= 1 + clip_param and 0 above,
 * d max(r, c)/dr is 1 for r >= 1 - clip_param and 0 below: what torch.autograd returns off the two clip edges.
 *
 * One preparation launch, then per network three kernels over ONE scratch that the second network reuses (the two-pass
 * form: the f32 MFMA fragments of one network's fc1 + fc2 fill 80 KB of a CU's 160 KB of LDS, both networks' do not fit):
 * A, the per-sample forward + backward on f32 MFMA; B, the weight-gradient contractions over the sample dimension, split
 * over workgroups that each write one partial block; C, the fold of the partial blocks in a fixed order.  No floating-point
 * atomics anywhere: two calls on the same inputs give bit-identical outputs.  Only enqueues work on `stream` (no
 * allocation, no synchronisation): graph-capturable.
 *
 * Exported by libmm_hip.so only (marl-mass_amd/csrc/mm_policy_train.hip), like mm_policy_gi_train: no oracle twin, not part
 * of include/mm_abi.h's symbol list or version.  torch.autograd on the two rollout modules is the CPU form.
 */
#ifndef MM_POLICY_TRAIN_H
#define MM_POLICY_TRAIN_H

#include <stdint.h>

#include "mm_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_PT_CRITIC_MSE 0
#define MM_PT_CRITIC_HUBER 1

/* The six parameter tensors of one network (or their gradients), torch nn.Linear layout [out][in], float32, DEV:
 *   actor:  W1 [128][n_s], b1 [128]; W2 [128][128],       b2 [128]; W3 [n_a][128], b3 [n_a]
 *   critic: W1 [128][n_s], b1 [128]; W2 [128][128 + n_a], b2 [128]; W3 [1][128],   b3 [1] */
typedef struct MMMlpParams {
  float *W1, *b1, *W2, *b2, *W3, *b3;
} MMMlpParams;

/*
 * Forward only, nothing sampled, no RNG counter: logp_taken[j] = actor(obs_j)[action_j] and / or value[j] =
 * critic(obs_j, one_hot(action_j)).  This is how old_logp (actor target) and the advantages (critic target) are obtained.
 * obs / actions / valid as in mm_policy_train.  actor with logp_taken, critic with value: either pair may be NULL (both
 * pointers of the pair), not both pairs.  Masked slots are not read and get 0.  n == 0 does nothing (the outputs may then be NULL).
 * MM_ERR_INVALID_ARG: as mm_policy_train, and a network given without its output or an output without its network.
 */
int32_t mm_policy_eval(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions, int64_t act_stride,
                       const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden, int32_t n_a,
                       float *logp_taken, float *value, MMStream stream);

/* Bytes of scratch mm_policy_train needs for n samples (n >= 0): 2 240 bytes per sample (x 32, h1, dz1, h2, dz2 128 each,
 * the head's gradient 16 floats; one network at a time, the critic's pass overwrites the actor's) plus 128 KB of transposed
 * fc2 fragments and up to 55 MB of partial blocks. */
int32_t mm_policy_train_scratch_bytes(int64_t n, uint64_t *bytes);

/*
 * obs: DEV float, sample j's row at obs + j * obs_stride (floats; >= n_s), 25 <= n_s <= 32.
 * actions: DEV int32, sample j at actions[j * act_stride]; a value outside 0..n_a-1 is the caller's error and is clamped.
 * returns: DEV float, sample j at returns[j * ret_stride] (read by the critic's pass only; may be NULL without a critic).
 * old_logp: DEV float[n], the actor target's log-probability of the taken action (actor's pass only).
 * valid: optional DEV uint8[n]; samples with valid[j] == 0 contribute nothing and are not counted in B (their obs / actions /
 * returns / old_logp / advantages are not read).
 * actor / critic: the parameters (read only); either may be NULL together with its gradients to get only the other's.
 * hidden must be 128; 1 <= n_a <= 8.   adv_sums / advantages: exactly one of them with an actor (see above).
 * actor_grads / critic_grads: six gradients each, WRITTEN (not accumulated).
 * loss: DEV float[2] = actor loss, critic loss (0 for an omitted network).
 * logp_taken / ratio (need the actor) / value (needs the critic): optional DEV float[n] diagnostics, 0 where valid[j] == 0.
 * scratch: DEV, scratch_bytes >= mm_policy_train_scratch_bytes(n), 16-byte aligned; contents are undefined afterwards.
 * n == 0 or no valid sample: gradients and losses are written as zeros (n == 0: the per-sample inputs, adv_sums and
 * advantages are not looked at and may be NULL).  n is limited to 2^31 - 1 (B is a 32-bit count).
 * The scratch is not chunked: 1.17 GiB at 524 288 samples; a caller with more samples than it can afford scratch for uses
 * mm_policy_train_chunked below (the same gradients of ONE loss per network over all n samples, in passes through the rows of
 * `chunk` samples).
 * MM_ERR_INVALID_ARG: no network at all, a network without gradients or the reverse, a NULL pointer among a given network's
 *   six, a NULL input the given networks read, loss NULL, n < 0, n > 2^31 - 1, n_s outside 25..32, obs_stride < n_s,
 *   hidden != 128, n_a outside 1..8, critic_loss not one of the two, clip_param < 0, with an actor both or neither of
 *   adv_sums / advantages, a diagnostic of an omitted network, scratch NULL / too small / misaligned.
 */
int32_t mm_policy_train(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions, int64_t act_stride,
                        const float *returns, int64_t ret_stride, const float *old_logp, const uint8_t *valid,
                        const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden, int32_t n_a, float clip_param,
                        int32_t critic_loss, const float *adv_sums, const float *advantages, const MMMlpParams *actor_grads,
                        const MMMlpParams *critic_grads, float *loss, float *logp_taken, float *value, float *ratio, void *scratch,
                        uint64_t scratch_bytes, MMStream stream);

/*
 * The same call under a fixed scratch budget (marl-mass_amd/csrc/mm_policy_chunked.hip), as mm_policy_gi_train_chunked
 * (include/mm_policy_gi_train.h) is to mm_policy_gi_train.  Kernels A and B run over the batch in passes of `chunk` samples,
 * the actor's pass and the critic's alternating over the same rows; each pass's partial blocks are added, in workgroup order and
 * in fp64, to the network's own accumulator block, and gradients and losses are written once at the end: the gradient of ONE
 * loss per network over all n samples, B the number of valid samples of the whole batch.  Deterministic, no floating-point
 * atomics, only enqueues on `stream`: graph-capturable.
 *
 * chunk: samples per pass, a positive multiple of 64.  Every other argument is mm_policy_train's.
 * Scratch (mm_policy_train_chunked_scratch_bytes(n, chunk), 16-byte aligned): the header and both networks' fragments as above,
 * the per-sample rows of `chunk` samples (2 240 bytes each), the fp64 loss partials of all ceil(n / 32) tiles (8 bytes per tile
 * and network: both networks' are folded at the end), the partial blocks of one pass (one per 2 tiles up to 1024 tiles, 512
 * above: up to 55 MB) and two accumulator blocks double[26 896].
 *
 * With chunk >= n the results are bit-identical to mm_policy_train; for any chunk the losses and the diagnostics are, and the
 * gradients differ from it only through the float32 rounding of a different slicing of the sample sum.
 * MM_ERR_INVALID_ARG: as mm_policy_train, and chunk <= 0 or not a multiple of 64.  A refused call enqueues nothing.
 */
int32_t mm_policy_train_chunked_scratch_bytes(int64_t n, int64_t chunk, uint64_t *bytes);

int32_t mm_policy_train_chunked(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden, int32_t n_a,
                                float clip_param, int32_t critic_loss, const float *adv_sums, const float *advantages,
                                const MMMlpParams *actor_grads, const MMMlpParams *critic_grads, float *loss, float *logp_taken,
                                float *value, float *ratio, void *scratch, uint64_t scratch_bytes, MMStream stream, int64_t chunk);

/*
 * The same gradients over a batch that is SHARDED over ranks, in two phases (marl-mass_amd/csrc/mm_policy_sharded.hip), as
 * mm_policy_gi_train_partial / mm_policy_gi_train_finish (include/mm_policy_gi_train.h: the protocol, the header's check and
 * the order of every sum are described there) are to mm_policy_gi_train_chunked.
 *
 * The shard block: MM_PT_SHARD_DOUBLES doubles on the device (mm_policy_train_shard_bytes gives the size in bytes),
 *   [0] B of the WHOLE batch   [1] this rank's own number of valid samples
 *   [2] the configuration word n_s + 2^8 n_a + 2^16 (reference form + 2 huber) + 2^24 networks (1 actor + 2 critic)   [3] 0
 *   [4] the un-normalised fp64 sum of the actor's loss terms, [5] of the critic's (0 for a network that was not given)
 *   [6 .. 6 + 26 896) the actor's fp64 accumulator block, then [.. + 26 896) the critic's, each in the layout of a kernel-B partial
 *       block (PartialBlock<4>, mm_policy_mfma.h): dW2 [128][160] at 0 (row pitch 160, k2 columns used); dW3 rows [16][128] at
 *       20 480; dW1 [128][32] at 22 528; db2 [128] at 26 624; db3 [16] at 26 752; db1 [128] at 26 768.  Zeros for a network
 *       that was not given.
 * Every double of the block is a function of the inputs: a slot that finish does not read (a dW2 column from k2 on, a dW3 row
 * or db3 element from the network's outputs on, a dW1 column from n_s on) is 0.0, whatever the scratch held.
 *
 * mm_policy_train_partial: mm_policy_train_chunked's arguments without actor_grads, critic_grads and loss, and with count (DEV
 * int32[1], 4-byte aligned: B of the whole batch over all ranks) and shard (DEV double[MM_PT_SHARD_DOUBLES], 16-byte aligned,
 * WRITTEN).  adv_sums is the whole batch's.  n == 0 writes a valid all-zero block with local count 0 (the per-sample pointers and
 * the scratch may be NULL).  scratch: mm_policy_train_chunked_scratch_bytes(n, chunk).
 * MM_ERR_INVALID_ARG: as mm_policy_train_chunked (without what concerns the gradients and loss), and count or shard NULL or
 * misaligned.  A refused call enqueues nothing.
 *
 * mm_policy_train_finish: actor_grads / critic_grads: the networks whose gradients are WRITTEN (at least one; the other's tensors
 * are not touched and its loss is 0).  loss: DEV float[2].  A requested network must be present in every block; that, and the
 * check of mm_policy_gi_train_finish, failing writes every requested gradient and both losses as NaN.  B == 0 writes zeros.
 * MM_ERR_INVALID_ARG: blocks or loss NULL, no gradients at all, a NULL pointer among a given network's six, n_blocks outside
 *   1..64, block_stride below the block size, n_s outside 25..32, n_a outside 1..8.
 */
#define MM_PT_SHARD_DOUBLES 53798 /* 4 + 2 + 2 * 26 896 */

int32_t mm_policy_train_shard_bytes(uint64_t *bytes);

int32_t mm_policy_train_partial(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden, int32_t n_a,
                                float clip_param, int32_t critic_loss, const float *adv_sums, const float *advantages,
                                const int32_t *count, double *shard, float *logp_taken, float *value, float *ratio, void *scratch,
                                uint64_t scratch_bytes, MMStream stream, int64_t chunk);

int32_t mm_policy_train_finish(const double *blocks, int32_t n_blocks, int64_t block_stride, int32_t n_s, int32_t n_a,
                               const MMMlpParams *actor_grads, const MMMlpParams *critic_grads, float *loss, MMStream stream);

#ifdef __cplusplus
}
#endif
#endif /* MM_POLICY_TRAIN_H */
