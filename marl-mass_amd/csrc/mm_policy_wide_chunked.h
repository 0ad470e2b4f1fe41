// mm_policy_wide_chunked.h -- how the entries of mm_policy_wide_train.hip and the pass loop of mm_policy_chunked.hip reach prep,
// kernel A and kernel B of mm_policy_wide_train.hip, and the layout they share: the scratch of n samples and the partial block of
// one slice.  Host-side launch helpers only, defined next to the kernels they launch (mm_policy_wide_train.hip) and the one
// spelling of each launch, for the unchunked entry (the whole batch) as for the chunked and the rank-sharded ones (a pass, through
// chunked::Pt512 of mm_policy_chunked.h): those add no __global__ to that file and edit none, so its code object stays as
// recorded (profiles/policy_wide_train).  A helper only enqueues on the stream; the caller reads hipGetLastError.
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

}  // namespace mm
#endif
