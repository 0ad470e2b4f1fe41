/*
 * mm_policy_wide_train.h -- loss and full parameter gradient of MAPPO's separate actor and critic at hidden size 512 (the
 * lateral_control = steer_vel configurations), and the forward-only mm_policy_wide_eval.
 *
 * It is include/mm_policy_train.h's contract at the other hidden size the reference trains with: the same networks
 * (Model_common.py:5-41), the same objective (one agent step of MAPPO.train(), marl/mappo.py:170-201, in its reference
 * [B, B] form through adv_sums or per sample through advantages), the same arguments, MMMlpParams and MM_PT_CRITIC_*:
 *   actor:  W1 [512][n_s], b1 [512]; W2 [512][512],       b2 [512]; W3 [n_a][512], b3 [n_a]
 *   critic: W1 [512][n_s], b1 [512]; W2 [512][512 + n_a], b2 [512]; W3 [1][512],   b3 [1]
 * mm_policy_train / mm_policy_eval keep refusing hidden != 128; these entries refuse hidden != 512.
 *
 * One preparation launch, then per network three kernels over ONE scratch that the second network reuses:
 *   A  per sample (one wave per MM_POLICY_WIDE_TRAIN_TILE samples, MM_POLICY_WIDE_TRAIN_WAVES waves per workgroup, at most
 *      MM_POLICY_WIDE_TRAIN_MAX_GRID persistent workgroups): fc1, fc2 (f32 MFMA, fc2's weight read from global memory), the
 *      head, the loss terms, dz2, and dz1 = (W2[:, :512]^T dz2) . [h1 > 0] (f32 MFMA against the transposed copy that the
 *      preparation launch wrote);
 *   B  dW2 = dz2^T [h1 | one_hot], dW3, dW1 (f32 MFMA, the sample index as the reduction) and the bias sums, split over
 *      slices of samples that each write one partial block;
 *   C  the fold of the partial blocks in slice order with an fp64 running sum.
 * No floating-point atomics anywhere: two calls on the same inputs give bit-identical outputs.  Only enqueues work on
 * `stream` (no allocation, no synchronisation): graph-capturable.
 *
 * mm_policy_wide_train_chunked (below) is the same gradient in passes under a fixed scratch budget, and
 * mm_policy_wide_train_partial / mm_policy_wide_train_finish (at the end) over a batch that is sharded over ranks.
 *
 * Exported by libmm_hip.so only (marl-mass_amd/csrc/mm_policy_wide_train.hip, mm_policy_chunked.hip, mm_policy_sharded.hip): no oracle twin, not part of
 * include/mm_abi.h's symbol list or version.  torch.autograd on the two rollout modules is the CPU form.
 */
#ifndef MM_POLICY_WIDE_TRAIN_H
#define MM_POLICY_WIDE_TRAIN_H

#include <stdint.h>

#include "mm_abi.h"
#include "mm_policy_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The decomposition of the launches, for callers that test their boundaries.  A row's diagnostics and mm_policy_wide_eval's
 * outputs depend on none of them. */
#define MM_POLICY_WIDE_TRAIN_TILE 32       /* samples per tile: one wave of kernel A owns one tile at a time */
#define MM_POLICY_WIDE_TRAIN_WAVES 8       /* waves per workgroup of kernel A */
#define MM_POLICY_WIDE_TRAIN_MAX_GRID 256  /* kernel A launches at most this many persistent workgroups */
/* Kernel B's slices are whole tiles: tiles_per_slice = max(MM_POLICY_WIDE_TRAIN_MIN_SLICE_TILES, ceil(ntiles /
 * MM_POLICY_WIDE_TRAIN_MAX_SLICES)), ntiles = ceil(n / 32), slices = ceil(ntiles / tiles_per_slice); the last slice is the
 * shorter one. */
#define MM_POLICY_WIDE_TRAIN_MAX_SLICES 48
#define MM_POLICY_WIDE_TRAIN_MIN_SLICE_TILES 2

/* The scratch, in bytes (what mm_policy_wide_train_scratch_bytes adds up):
 *   MM_POLICY_WIDE_TRAIN_FIXED_BYTES   a 256-byte header (the count of valid samples) and four [512][512] float blocks:
 *                                      W2[:, :512]^T of the actor and of the critic for dz1, and a copy of each network's
 *                                      W2[:, :512] at row pitch 512 (used in place of W2 where its rows are not 16-byte
 *                                      aligned, as the critic's are for n_a = 5)
 *   MM_POLICY_WIDE_TRAIN_ROW_BYTES     per sample of the n rounded up to whole tiles: x (32 floats), h1, h2, dz2, dz1 (512
 *                                      each) and the head's gradient (16); one network at a time
 *   8 bytes per tile                   the fp64 loss partial
 *   MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES per slice: dW2 [512][544], the head rows [16][512], dW1 [512][32], the bias sums
 *                                      [512 + 16 + 512]; at most MM_POLICY_WIDE_TRAIN_MAX_SLICES of them, which is the
 *                                      upper bound MM_POLICY_WIDE_TRAIN_PARTIAL_MAX_BYTES (58.4 MB) */
#define MM_POLICY_WIDE_TRAIN_FIXED_BYTES (256 + 4 * 512 * 512 * 4)
#define MM_POLICY_WIDE_TRAIN_ROW_BYTES ((32 + 4 * 512 + 16) * 4)
#define MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES ((512 * 544 + 16 * 512 + 512 * 32 + 512 + 16 + 512) * 4)
#define MM_POLICY_WIDE_TRAIN_PARTIAL_MAX_BYTES (MM_POLICY_WIDE_TRAIN_MAX_SLICES * MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES)

/* Alignment: none beyond mm_policy_train's.  The scratch is MM_POLICY_WIDE_TRAIN_SCRATCH_ALIGN-byte aligned (an argument
 * error otherwise); every other pointer needs its element's alignment only.  fc2's weight is read with 16-byte loads where
 * its rows allow (pointer and row length multiples of 16 bytes) and with 4-byte loads otherwise -- the same values in the
 * same order, so the outputs do not depend on which. */
#define MM_POLICY_WIDE_TRAIN_SCRATCH_ALIGN 16

/*
 * mm_policy_eval's contract (include/mm_policy_train.h) at hidden == 512: logp_taken[j] = actor(obs_j)[action_j] and / or
 * value[j] = critic(obs_j, one_hot(action_j)); masked slots are not read and get 0; n == 0 does nothing.  A row's outputs
 * are a function of that row and the weights alone: not of n, nor of where the row falls in the launch, and they equal the
 * diagnostics mm_policy_wide_train writes for the same row bit for bit.  Needs no scratch.
 * MM_ERR_INVALID_ARG: as mm_policy_eval, with hidden != 512 in place of hidden != 128.
 */
int32_t mm_policy_wide_eval(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                            int64_t act_stride, const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic,
                            int32_t hidden, int32_t n_a, float *logp_taken, float *value, MMStream stream);

/* Bytes of scratch mm_policy_wide_train needs for n samples (n >= 0), monotone in n: the sum stated above.  Host arithmetic. */
int32_t mm_policy_wide_train_scratch_bytes(int64_t n, uint64_t *bytes);

/*
 * mm_policy_train's arguments and contract (include/mm_policy_train.h) with hidden == 512: both actor forms, the optional
 * valid mask, strides and diagnostics, gradients WRITTEN (not accumulated), loss float[2], either network omitted together
 * with its gradients, n == 0 or no valid sample writes zeros.  Gradient rows of masked or out-of-range samples are exact
 * zeros and a masked sample's inputs are not read.
 * The scratch is not chunked: 4.15 GiB at 524 288 samples; a caller with more samples than it can afford scratch for uses
 * mm_policy_wide_train_chunked below (the same gradients of ONE loss per network over all n samples, in passes through the
 * rows of `chunk` samples).
 * MM_ERR_INVALID_ARG: every case of mm_policy_train, with hidden != 512 in place of hidden != 128, scratch NULL, smaller
 * than mm_policy_wide_train_scratch_bytes(n) or off MM_POLICY_WIDE_TRAIN_SCRATCH_ALIGN.  A refused call enqueues nothing and
 * writes nothing.
 */
int32_t mm_policy_wide_train(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                             int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                             const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden,
                             int32_t n_a, float clip_param, int32_t critic_loss, const float *adv_sums, const float *advantages,
                             const MMMlpParams *actor_grads, const MMMlpParams *critic_grads, float *loss, float *logp_taken,
                             float *value, float *ratio, void *scratch, uint64_t scratch_bytes, MMStream stream);

/*
 * The same call under a fixed scratch budget (marl-mass_amd/csrc/mm_policy_chunked.hip): mm_policy_train_chunked's
 * contract (include/mm_policy_train.h) at hidden == 512.  Kernels A and B run over the batch in passes of `chunk` samples, the
 * actor's pass and the critic's alternating over the same rows; each pass's partial blocks are added, in slice order and in
 * fp64, to the network's own accumulator block, and gradients and losses are written once at the end: the gradient of ONE
 * loss per network over all n samples, B the number of valid samples of the whole batch, formed by the one preparation
 * launch.  Deterministic, no floating-point atomics, only enqueues on `stream`: graph-capturable.
 *
 * chunk: samples per pass, a positive multiple of 64.  Every other argument is mm_policy_wide_train's.
 * Scratch (mm_policy_wide_train_chunked_scratch_bytes(n, chunk), MM_POLICY_WIDE_TRAIN_SCRATCH_ALIGN-byte aligned), the sum
 * MM_POLICY_WIDE_TRAIN_CHUNKED_BYTES(n, chunk) of
 *   MM_POLICY_WIDE_TRAIN_FIXED_BYTES                      as above
 *   chunk * MM_POLICY_WIDE_TRAIN_ROW_BYTES                the rows of one pass
 *   MM_POLICY_WIDE_TRAIN_CHUNKED_LOSS_BYTES per tile      the fp64 loss partials of all ceil(n / 32) tiles of BOTH networks
 *                                                         (both are folded at the end): all that grows with n
 *   MM_POLICY_WIDE_TRAIN_CHUNKED_BLOCKS(chunk) blocks     of MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES: the partial blocks of one pass.
 *                                                         The most slices ANY pass of at most `chunk` samples cuts, not the
 *                                                         slices of a full pass: under the slicing rule above a shorter last
 *                                                         pass can cut more (chunk 3136 = 98 tiles: 33 slices of 3 tiles; a
 *                                                         last pass of 3072 samples = 96 tiles: 48 slices of 2)
 *   2 * MM_POLICY_WIDE_TRAIN_ACC_BYTES                    one accumulator block double[MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES / 4]
 *                                                         per network
 * 10.8 MB for the smallest call (64 samples in one pass): the fixed part and the two accumulators.
 *
 * With chunk >= n the results are bit-identical to mm_policy_wide_train; for any chunk the losses and the diagnostics are,
 * and the gradients differ from it only through the float32 rounding of a different slicing of the sample sum.  n == 0 or no
 * valid sample: as mm_policy_wide_train.
 * MM_ERR_INVALID_ARG: as mm_policy_wide_train (the scratch against the chunked size), and chunk <= 0 or not a multiple of 64.
 * A refused call enqueues nothing and writes nothing.
 */
#define MM_POLICY_WIDE_TRAIN_CHUNKED_LOSS_BYTES 16
#define MM_POLICY_WIDE_TRAIN_ACC_BYTES (2 * MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES)
#define MM_POLICY_WIDE_TRAIN_CHUNKED_BLOCKS(chunk) \
  ((chunk) / 64 < MM_POLICY_WIDE_TRAIN_MAX_SLICES ? (chunk) / 64 : MM_POLICY_WIDE_TRAIN_MAX_SLICES)
#define MM_POLICY_WIDE_TRAIN_CHUNKED_BYTES(n, chunk)                                                                          \
  ((uint64_t)MM_POLICY_WIDE_TRAIN_FIXED_BYTES + (uint64_t)(chunk) * MM_POLICY_WIDE_TRAIN_ROW_BYTES +                            \
   (((uint64_t)(n) + 31) / 32) * MM_POLICY_WIDE_TRAIN_CHUNKED_LOSS_BYTES +                                                      \
   (uint64_t)MM_POLICY_WIDE_TRAIN_CHUNKED_BLOCKS(chunk) * MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES + 2 * (uint64_t)MM_POLICY_WIDE_TRAIN_ACC_BYTES)

int32_t mm_policy_wide_train_chunked_scratch_bytes(int64_t n, int64_t chunk, uint64_t *bytes);

int32_t mm_policy_wide_train_chunked(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                     int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                     const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden,
                                     int32_t n_a, float clip_param, int32_t critic_loss, const float *adv_sums,
                                     const float *advantages, const MMMlpParams *actor_grads, const MMMlpParams *critic_grads,
                                     float *loss, float *logp_taken, float *value, float *ratio, void *scratch,
                                     uint64_t scratch_bytes, MMStream stream, int64_t chunk);

/*
 * The same gradients over a batch that is SHARDED over ranks, in two phases (marl-mass_amd/csrc/mm_policy_sharded.hip):
 * mm_policy_train_partial / mm_policy_train_finish's protocol (include/mm_policy_train.h; the header's check and the order of
 * every sum: include/mm_policy_gi_train.h) at hidden == 512, as those are to mm_policy_train_chunked.  Every rank runs `partial`
 * on its own samples, the R blocks are gathered in rank order, and every rank runs `finish` on the same R blocks: the same bits
 * on every rank.
 *
 * The shard block: MM_PW_SHARD_DOUBLES doubles on the device, 16-byte aligned, 4 866 352 bytes (mm_policy_wide_train_shard_bytes),
 *   [0] B of the WHOLE batch   [1] this rank's own number of valid samples
 *   [2] the configuration word n_s + 2^8 n_a + 2^16 (reference form + 2 huber) + 2^24 networks (1 actor + 2 critic) + 2^26; the
 *       2^26 bit says "hidden 512": an exact integer below 2^31, and a hidden-128 block never passes the wide finish   [3] 0
 *   [4] the un-normalised fp64 sum of the actor's loss terms, [5] of the critic's (0 for a network that was not given)
 *   [6 .. 6 + 304 144) the actor's fp64 accumulator block, then [.. + 304 144) the critic's, each in the layout of one kernel-B
 *       partial block (MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES / 4 slots): dW2 [512][544] at 0 (row pitch 544, k2 columns used: 512
 *       for the actor, 512 + n_a for the critic); head rows [16][512] at 278 528 (n_a rows used, 1 for the critic); dW1 [512][32]
 *       at 286 720 (n_s columns used); db2 [512] at 303 104; head bias [16] at 303 616; db1 [512] at 303 632.  Zeros for a
 *       network that was not given.
 * Every double of the block is a function of the inputs: a slot that finish does not read (a column, row or bias beyond the
 * used ones above) is 0.0, whatever the scratch held.
 *
 * mm_policy_wide_train_partial: mm_policy_wide_train_chunked's arguments without actor_grads, critic_grads and loss, and with
 * count (DEV int32[1], 4-byte aligned: B of the whole batch over all ranks) and shard (DEV double[MM_PW_SHARD_DOUBLES], 16-byte
 * aligned, WRITTEN).  Kernel A scales by *count; adv_sums is the whole batch's.  Kernel A, the loss tree and the pass and slice
 * order are the chunked entry's.  n == 0 writes a valid all-zero block with local count 0 (the per-sample pointers and the
 * scratch may be NULL).  scratch: mm_policy_wide_train_chunked_scratch_bytes(n, chunk); its two accumulator blocks go unused.
 * MM_ERR_INVALID_ARG: as mm_policy_wide_train_chunked (without what concerns the gradients and loss), count or shard NULL or
 * misaligned, hidden != 512.  A refused call enqueues nothing.
 *
 * mm_policy_wide_train_finish: actor_grads / critic_grads: the networks whose gradients are WRITTEN (at least one; the other's
 * tensors are not touched and its loss is 0).  loss: DEV float[2].  One thread per gradient element starts from block 0's
 * value, adds blocks 1 .. n_blocks - 1 in index order in fp64 and rounds once to float32; the losses are the R loss doubles
 * added in index order and scaled as the chunked entry scales them (-s / B, reference form -s / B^2; critic s / B).  Every block
 * must carry the same B and configuration word, the word must be that of the call (n_s, n_a, the hidden-512 bit) and name every
 * requested network, and the local counts must add up to B: if not, every requested gradient and both losses are NaN.
 * B == 0 writes zeros.  With one block and B the rank's own count the results are mm_policy_wide_train_chunked's bits.
 * MM_ERR_INVALID_ARG: blocks or loss NULL, no gradients at all, a NULL pointer among a given network's six, n_blocks outside
 *   1..64, block_stride below MM_PW_SHARD_DOUBLES, n_s outside 25..32, n_a outside 1..8.
 * Both: deterministic, no floating-point atomics, only enqueue on `stream`: graph-capturable.
 */
#define MM_PW_SHARD_DOUBLES 608294 /* 4 + 2 + 2 * 304 144 */

int32_t mm_policy_wide_train_shard_bytes(uint64_t *bytes);

int32_t mm_policy_wide_train_partial(const float *obs, int64_t obs_stride, int64_t n, int32_t n_s, const int32_t *actions,
                                     int64_t act_stride, const float *returns, int64_t ret_stride, const float *old_logp,
                                     const uint8_t *valid, const MMMlpParams *actor, const MMMlpParams *critic, int32_t hidden,
                                     int32_t n_a, float clip_param, int32_t critic_loss, const float *adv_sums,
                                     const float *advantages, const int32_t *count, double *shard, float *logp_taken, float *value,
                                     float *ratio, void *scratch, uint64_t scratch_bytes, MMStream stream, int64_t chunk);

int32_t mm_policy_wide_train_finish(const double *blocks, int32_t n_blocks, int64_t block_stride, int32_t n_s, int32_t n_a,
                                    const MMMlpParams *actor_grads, const MMMlpParams *critic_grads, float *loss, MMStream stream);

#ifdef __cplusplus
}
#endif
#endif /* MM_POLICY_WIDE_TRAIN_H */
