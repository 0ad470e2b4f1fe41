// mm_policy_wide_chunked.h -- how the entries of mm_policy_wide_train.hip and mm_policy_wide_chunked.hip reach prep, kernel A and
// kernel B of mm_policy_wide_train.hip, and the layout the two files share: the scratch of n samples and the partial block of one
// slice; and what the chunked entry and the rank-sharded ones (mm_policy_wide_sharded.hip) share (at the end).  Host-side launch helpers only, defined next to the kernels they launch (mm_policy_wide_train.hip) and the one spelling
// of each launch, for the unchunked entry (the whole batch) as for the chunked one (a pass): the chunked entry adds no __global__
// to that file and edits none, so its code object stays as recorded (profiles/policy_wide_train).  A helper only enqueues on the
// stream; the caller reads hipGetLastError.
#ifndef MM_POLICY_WIDE_CHUNKED_H
#define MM_POLICY_WIDE_CHUNKED_H
#include "mm_policy_mfma.h"
#include "../../include/mm_policy_wide_train.h"

namespace mm {
namespace wt {

constexpr int kWide = 512;                               // hidden size
constexpr int kCat = kWide + 32;                         // row pitch of the dW2 partial: 512 + the one-hot tile
constexpr long long kSquare = (long long)kWide * kWide;  // floats of one [512][512] block

// the partial block of one slice, in floats
struct Part {
  static constexpr int kW2 = 0;                      // [512][544]
  static constexpr int kHd = kW2 + kWide * kCat;     // [16][512]: head rows
  static constexpr int kW1 = kHd + 16 * kWide;       // [512][32]: dz1^T x, all columns
  static constexpr int kb2 = kW1 + kWide * 32;       // [512]
  static constexpr int kbh = kb2 + kWide;            // [16]
  static constexpr int kb1 = kbh + 16;               // [512]
  static constexpr int kSize = kb1 + kWide;
};

// The scratch of a call on n samples, offsets in floats
struct WideLayout {
  long long n_pad, ntiles;
  long long w2t, w2p, xs, h1, h2, dz2, dz1, dh, lossp, part, total;  // w2t / w2p: the actor's block, then the critic's
  int slices;
  long long slice_rows;
};

// the per-sample rows of the scratch that kernel A writes and kernel B reads
struct WideRows {
  float *xs, *h1, *h2, *dz2, *dz1, *dh;
};

// the per-sample inputs and outputs of one launch of kernel A (train form): n samples starting at these pointers
struct PassArgs {
  const float *obs;
  long long obs_stride, n;
  int n_s;
  const int32_t *actions;
  long long act_stride;
  const float *returns;
  long long ret_stride;
  const float *old_logp;
  const uint8_t *valid;
  MMMlpParams w;
  int n_a;
  float clip_param;
  int huber;
  const float *adv_sums, *advantages;
  const int *count;
  const float *w2t, *w2p;  // this network's two [512][512] blocks that prep wrote: W2[:, :512]^T and W2[:, :512] at pitch 512
  WideRows rows;
  double *lossp;
  float *out0, *out1;  // actor: logp_taken, ratio; critic: value, unused
};

WideLayout layout_of(long long n);  // the unchunked scratch of n samples
void launch_prep(hipStream_t s, const float *W2a, const float *W2c, int k2c, float *w2t, float *w2p, const uint8_t *valid, long long n,
                 int *count);
// fc2's A operand is w.W2 in place where its rows take 16-byte loads, else the copy at pitch 512: the unchunked entry's choice
void launch_sample(hipStream_t s, bool critic, const PassArgs &p);
void launch_wgrad(hipStream_t s, bool critic, const WideRows &r, long long n_pad, long long slice_rows, int slices, float *part);

}  // namespace wt

// ---- what the chunked entry (mm_policy_wide_chunked.hip) and the rank-sharded ones (mm_policy_wide_sharded.hip) share: the
// chunked scratch layout, the argument check and the pass loop, defined in mm_policy_wide_chunked.hip next to the accumulate
// kernel the loop launches
namespace wide_chunked {

// The chunked scratch, offsets in floats: the header, the four [512][512] blocks and the per-sample rows as in the unchunked
// layout of `chunk` samples; then the fp64 loss partials of all ceil(n / 32) tiles of the actor and of the critic, the partial
// blocks of one pass, and the two fp64 accumulator blocks (the sharded entries accumulate into the caller's shard block and leave
// them unused).
// The partial blocks hold the most slices ANY pass of at most `chunk` samples cuts, not the slices of a full pass: under the
// header's rule a pass of t tiles cuts ceil(t / max(2, ceil(t / 48))) slices, never more than 48 nor than ceil(t / 2), and a
// shorter last pass can cut more than a full one (98 tiles: 33 slices of 3; 96 tiles: 48 slices of 2).
struct ChunkLayout {
  wt::WideLayout rows;  // the unchunked layout of `chunk` samples: w2t, w2p, xs .. dh
  long long ntiles, lossp, part, acc, total;
  int blocks;
};

// one network of a call (NULL w: not given) and its per-sample outputs: logp_taken, ratio | value, unused
struct WideNet {
  const MMMlpParams *w;
  float *out0, *out1;
};

// What the chunked and the partial entry refuse alike, on the whole batch's PassArgs (n the whole batch, the pointers at sample
// 0): the weights, the shape limits, critic_loss, clip_param, chunk, diagnostics without their network and, when n > 0, the
// per-sample inputs, adv_sums against advantages, and the scratch: its pointer, alignment and size, and that the two pass sizes
// there are, the full one and the last one's, fit the rows and the partial blocks the size query promised.  Enqueues nothing.
// L: the scratch layout when n > 0.
bool wide_args_ok(const wt::PassArgs &batch, const WideNet (&net)[2], int32_t hidden, int32_t critic_loss, int64_t chunk,
                  const void *scratch, uint64_t scratch_bytes, ChunkLayout &L);

// The passes of a batch of n > 0 samples that the check above let through: prep once over the whole batch (its count of valid
// samples goes to the scratch header, the int at sc, which the caller has zeroed), then per pass of `chunk` samples and per
// network, the actor first, kernel A (scaled by batch.count), kernel B and accumulate through the rows of the scratch at sc, the
// per-sample pointers of a copy of `batch` shifted on the host.  The critic's accumulator follows the actor's
// (acc + wt::Part::kSize); the loss partials are the actor's double[ntiles] at sc + L.lossp, then the critic's.
void wide_passes(hipStream_t s, const wt::PassArgs &batch, const WideNet (&net)[2], long long chunk, const ChunkLayout &L, float *sc,
                 double *acc);

}  // namespace wide_chunked
}  // namespace mm
#endif
