/*
 * mm_policy_gi_train.h -- loss and full parameter gradient of MAPPO_GI's shared actor-critic (shared_network = True).
 *
 * The network is the one of include/mm_policy_gi.h (Model_gi.ActorCriticNetwork(state_split=True), hidden 128); the
 * objective is the shared branch of MAPPO_GI.train() (marl/mappo_gi.py:305-339) for ONE batch of samples:
 *
 *   logp_j  = log_softmax(actor_linear(trunk(obs_j)))[action_j]         value_j = critic_linear(trunk(obs_j))
 *   r_j     = exp(logp_j - old_logp_j)                                  c_j = clip(r_j, 1 - clip_param, 1 + clip_param)
 *   critic  = (1 / B) sum_j l(value_j - returns_j)       l(d) = d^2 (MM_GI_CRITIC_MSE) | smooth_l1, beta = 1 (MM_GI_CRITIC_HUBER)
 *   actor   = one of two forms, chosen by adv_sums:
 *     adv_sums != NULL  the reference's own arithmetic.  There `ratio` is [B] and `advantages = returns - values.detach()`
 *                       is [B, 1], so `ratio * advantages` broadcasts to [B, B] and the loss is
 *                       -mean_{i,j} min(r_j A_i, c_j A_i) = -(1 / B^2) sum_j [S+ min(r_j, c_j) + S- max(r_j, c_j)],
 *                       S+ = sum of the non-negative A_i, S- = sum of the negative A_i: adv_sums = DEV float[2] {S+, S-}
 *                       (the caller gets them from a value-only mm_policy_gi_act pass and two reductions).
 *     adv_sums == NULL  textbook PPO-clip: -(1 / B) sum_j min(r_j A_j, c_j A_j), A_j = returns_j - value_j with value_j
 *                       from this launch's own forward, detached.
 *   loss = actor + critic; its gradient reaches the shared trunk from both heads.
 * B is the number of valid samples (valid == NULL: n).  d min(r, c)/dr is 1 for r <= 1 + clip_param and 0 above,
 * d max(r, c)/dr is 1 for r >= 1 - clip_param and 0 below: what torch.autograd returns off the two clip edges.
 *
 * Three kernels after a small preparation launch: A, the per-sample forward + backward on f32 MFMA (activations and their
 * gradients go to `scratch` in [sample][feature] order); B, the weight-gradient contractions over the sample dimension,
 * split over workgroups that each write one partial block; C, the fold of the partial blocks in a fixed order.  No
 * floating-point atomics anywhere: two calls on the same inputs give bit-identical outputs.  Only enqueues work on
 * `stream` (no allocation, no synchronisation): graph-capturable.
 *
 * Exported by libmm_hip.so only (marl-mass_amd/csrc/mm_policy_gi_train.hip), like mm_policy_gi_act: no oracle twin, not
 * part of include/mm_abi.h's symbol list or version.  torch.autograd on rollout.ActorCriticNetwork is the CPU form.
 */
#ifndef MM_POLICY_GI_TRAIN_H
#define MM_POLICY_GI_TRAIN_H

#include <stdint.h>

#include "mm_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_GI_CRITIC_MSE 0
#define MM_GI_CRITIC_HUBER 1

/* The twelve parameter tensors of the network (or their gradients), torch nn.Linear layout [out][in], float32, DEV:
 *   W11 [32][5], b11 [32]; W12 [64][10], b12 [64]; W13 [64][10], b13 [64]; W2 [128][160], b2 [128];
 *   Wa [n_a][128], ba [n_a]; Wc [1][128], bc [1]. */
typedef struct MMGiParams {
  float *W11, *b11, *W12, *b12, *W13, *b13, *W2, *b2, *Wa, *ba, *Wc, *bc;
} MMGiParams;

/* Bytes of scratch mm_policy_gi_train needs for n samples (n >= 0). */
int32_t mm_policy_gi_train_scratch_bytes(int64_t n, uint64_t *bytes);

/*
 * obs: DEV float, sample j's row at obs + j * obs_stride (floats; >= n_s), 25 <= n_s <= 32 (columns 0..24 are read).
 * actions: DEV int32, sample j at actions[j * act_stride]; a value outside 0..n_a-1 is the caller's error and is clamped.
 * returns: DEV float, sample j at returns[j * ret_stride].   old_logp: DEV float[n], the target network's log-probability of
 * the taken action.   valid: optional DEV uint8[n]; samples with valid[j] == 0 contribute nothing and are not counted in B
 * (their obs / actions / returns / old_logp are not read).
 * weights: the network's parameters (read only).   hidden must be 128; 1 <= n_a <= 8.
 * grads: the twelve gradients, WRITTEN (not accumulated).   loss: DEV float[3] = actor loss, critic loss, their sum.
 * logp_taken / value / ratio: optional DEV float[n] diagnostics (0 where valid[j] == 0).
 * scratch: DEV, scratch_bytes >= mm_policy_gi_train_scratch_bytes(n), 16-byte aligned; contents are undefined afterwards.
 * n == 0 or no valid sample: gradients and losses are written as zeros.  n is limited to 2^31 - 1 (B is a 32-bit count).
 * The scratch is 2 496 bytes per sample plus up to 56 MB of partial blocks and is not chunked: 1.27 GiB at 524 288 samples;
 * a caller with more samples than it can afford scratch for uses mm_policy_gi_train_chunked below (the same gradient of ONE
 * loss over all n samples, in passes through the rows of `chunk` samples).
 * MM_ERR_INVALID_ARG: a NULL input, weight or output pointer, n < 0, n_s outside 25..32, obs_stride < n_s, hidden != 128,
 *   n > 2^31 - 1, n_a outside 1..8, critic_loss not one of the two, clip_param < 0, scratch NULL / too small / misaligned.
 */
int32_t mm_policy_gi_train(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                           int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                           const uint8_t *valid, const MMGiParams *weights, int32_t hidden, int32_t n_a, float clip_param,
                           int32_t critic_loss, const float *adv_sums, const MMGiParams *grads, float *loss, float *logp_taken,
                           float *value, float *ratio, void *scratch, uint64_t scratch_bytes, MMStream stream);

/*
 * The same call under a fixed scratch budget (marl-mass_amd/csrc/mm_policy_chunked.hip).  Kernels A and B run over the batch
 * in passes of `chunk` samples through one set of per-sample rows; each pass's partial blocks are added, in workgroup order and
 * in fp64, to one accumulator block, and gradients and losses are written once at the end.  They mean what they mean above:
 * the gradient of ONE loss over all n samples, B the number of valid samples of the whole batch.  Deterministic, no
 * floating-point atomics, only enqueues on `stream` (1 + 3 launches per pass + 1, and two memsets): graph-capturable.
 *
 * chunk: samples per pass, a positive multiple of 64 (every pass but the last is whole 32-sample tiles, and a slice of kernel B
 * keeps its 2 tiles).  Every other argument is mm_policy_gi_train's.
 * Scratch (mm_policy_gi_train_chunked_scratch_bytes(n, chunk), 16-byte aligned): the header and the W2^T fragments as above,
 * the per-sample rows of `chunk` samples (2 496 bytes each), the fp64 loss partials of all ceil(n / 32) tiles (16 bytes each),
 * the partial blocks of one pass (one per 2 tiles up to 1024 tiles, 512 above: up to 56 MB) and one accumulator block
 * double[27 952].  At chunk 524 288 that is 1.27 GiB + 0.5 MB per million samples, whatever n.
 *
 * A gradient element is float(the fp64 running sum of all partial blocks of all passes, in pass and workgroup order), which is
 * what the unchunked fold computes over its one pass.  So with chunk >= n the results are bit-identical to mm_policy_gi_train;
 * for any chunk the losses and the diagnostics are (same tiles, same B, same loss tree), and the gradients differ from it only
 * through the float32 rounding of a different slicing of the sample sum.
 * MM_ERR_INVALID_ARG: as mm_policy_gi_train, and chunk <= 0 or not a multiple of 64.  A refused call enqueues nothing.
 */
int32_t mm_policy_gi_train_chunked_scratch_bytes(int64_t n, int64_t chunk, uint64_t *bytes);

int32_t mm_policy_gi_train_chunked(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                   int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                   const uint8_t *valid, const MMGiParams *weights, int32_t hidden, int32_t n_a, float clip_param,
                                   int32_t critic_loss, const float *adv_sums, const MMGiParams *grads, float *loss,
                                   float *logp_taken, float *value, float *ratio, void *scratch, uint64_t scratch_bytes,
                                   MMStream stream, int64_t chunk);

/*
 * The same gradient over a batch that is SHARDED over ranks, in two phases (marl-mass_amd/csrc/mm_policy_sharded.hip).  Every
 * rank runs `partial` on its own samples and leaves a shard block; the R blocks are gathered (the caller's collective) and
 * `finish` folds them, on every rank in the same order, into the gradient of ONE loss over all ranks' samples.
 *
 * The shard block: MM_GI_SHARD_DOUBLES doubles on the device (mm_policy_gi_train_shard_bytes gives the size in bytes),
 *   [0] B, the number of valid samples of the WHOLE batch   [1] this rank's own number of valid samples
 *   [2] the configuration word n_s + 2^8 n_a + 2^16 (reference form + 2 huber) + 2^24 networks (networks = 3)   [3] 0
 *   [4] [5] the un-normalised fp64 sums of the actor and the critic loss terms of this rank's samples
 *   [6 .. 6 + 27 952)  the fp64 accumulator block, in the layout of a kernel-B partial block (PartialBlock<5>, mm_policy_mfma.h):
 *       dW2 [128][160] at 0; the head rows [16][128] at 20 480 (rows 0..7 dWa, row 8 dWc); dW1 [160][32] at 22 528 (rows 0..31
 *       fc11, whose column k is column 5 k; rows 32..95 fc12, column k at 5 (k / 2) + 1 + k % 2; rows 96..159 fc13, column k at
 *       5 (k / 2) + 3 + k % 2); db2 [128] at 27 648; the heads' biases [16] at 27 776 (0..7 ba, 8 bc); db1 [160] at 27 792
 *       (fc11, fc12, fc13 in the rows' order).
 *
 * mm_policy_gi_train_partial: mm_policy_gi_train_chunked's arguments without grads and loss, and with
 *   count   DEV int32[1], 4-byte aligned: B of the whole batch over all ranks.  Kernel A scales by it; the entry does not compute it.
 *   shard   DEV double[MM_GI_SHARD_DOUBLES], 16-byte aligned: WRITTEN.
 * adv_sums (reference form) is likewise the whole batch's (S+, S-).  The entry zeroes the block, runs prep (the W2^T fragments and
 * the rank's own count), the chunked entry's passes of `chunk` samples with the accumulation going straight into the block, and
 * one kernel that folds the rank's loss partials (the chunked finish's tree) into [4], [5] and writes the header.  The diagnostics
 * are written as mm_policy_gi_train_chunked writes them.  n == 0 (an empty shard: the per-sample pointers and the scratch may be
 * NULL) writes a valid all-zero block with local count 0.  scratch: mm_policy_gi_train_chunked_scratch_bytes(n, chunk).
 * MM_ERR_INVALID_ARG: as mm_policy_gi_train_chunked, and count or shard NULL or misaligned.  A refused call enqueues nothing.
 *
 * mm_policy_gi_train_finish: blocks DEV double, block r at blocks + r * block_stride (doubles; >= MM_GI_SHARD_DOUBLES),
 * 1 <= n_blocks <= 64.  One launch: gradient element e = float(block 0's value + block 1's + ... + block R-1's, in index order,
 * fp64), written in torch layout; loss[0] = -(sum_r [4]) / B (per-sample form) or / B^2 (reference form), loss[1] = (sum_r [5]) / B,
 * loss[2] their float32 sum, the sums in index order.  With one block whose B is its own count these are
 * mm_policy_gi_train_chunked's bits for the same chunk.  The launch checks the headers: every block carries the same B and
 * configuration word, the word is that of n_s and n_a, and the local counts add up to B; if not, ALL gradients and losses are
 * written as NaN (a wrong B never becomes a plausible gradient).  B == 0 writes zeros.  No floating-point atomics; only enqueues
 * on `stream`.
 * MM_ERR_INVALID_ARG: blocks, grads (or one of its twelve) or loss NULL, n_blocks outside 1..64, block_stride below the block
 *   size, n_s outside 25..32, n_a outside 1..8.
 */
#define MM_GI_SHARD_DOUBLES 27958 /* 4 + 2 + 27 952 */

int32_t mm_policy_gi_train_shard_bytes(uint64_t *bytes);

int32_t mm_policy_gi_train_partial(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                   int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                   const uint8_t *valid, const MMGiParams *weights, int32_t hidden, int32_t n_a, float clip_param,
                                   int32_t critic_loss, const float *adv_sums, const int32_t *count, double *shard,
                                   float *logp_taken, float *value, float *ratio, void *scratch, uint64_t scratch_bytes,
                                   MMStream stream, int64_t chunk);

int32_t mm_policy_gi_train_finish(const double *blocks, int32_t n_blocks, int64_t block_stride, int32_t n_s, int32_t n_a,
                                  const MMGiParams *grads, float *loss, MMStream stream);

#ifdef __cplusplus
}
#endif
#endif /* MM_POLICY_GI_TRAIN_H */
