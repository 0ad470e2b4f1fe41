// mm_policy_chunked.h -- how mm_policy_chunked.hip reaches prep, kernel A and kernel B of the two training files.
// Host-side launch helpers only, defined next to the kernels they launch (mm_policy_gi_train.hip, mm_policy_train.hip): the
// chunked entries add no __global__ to those files and edit none, so their code objects stay as recorded
// (profiles/policy_gi_train, profiles/policy_train).  A helper only enqueues on the stream; the caller reads hipGetLastError.
#ifndef MM_POLICY_CHUNKED_H
#define MM_POLICY_CHUNKED_H
#include "mm_policy_mfma.h"
#include "../../include/mm_policy_gi_train.h"
#include "../../include/mm_policy_train.h"

namespace mm {

// the per-sample rows of the scratch that kernel A writes and kernel B reads
struct SampleRows {
  float *h1, *dz1, *h2, *dz2, *dh, *xs;
};

namespace gi_train {

// the per-sample inputs and outputs of one launch of kernel A: n samples starting at these pointers
struct PassArgs {
  const float *obs;
  long long obs_stride, n;
  const int32_t *actions;
  long long act_stride;
  const float *returns;
  long long ret_stride;
  const float *old_logp;
  const uint8_t *valid;
  MMGiParams w;
  int n_a;
  float clip_param;
  int huber;
  const float *adv_sums;
  const int *count;
  const float4 *frag;
  SampleRows rows;
  double *lossp;
  float *logp_out, *value_out, *ratio_out;
};

mfma::Layout layout_of(long long n);  // the unchunked scratch of n samples
void launch_prep(hipStream_t s, const float *W2, float4 *frag, const uint8_t *valid, long long n, int *count);
void launch_sample(hipStream_t s, const PassArgs &p);
void launch_wgrad(hipStream_t s, const SampleRows &r, long long n_pad, long long slice_rows, int slices, float *part);

}  // namespace gi_train

namespace pt {

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
  const float4 *frag;
  SampleRows rows;
  double *lossp;
  float *out0, *out1;  // actor: logp_taken, ratio; critic: value, unused
};

mfma::Layout layout_of(long long n);  // the unchunked scratch of n samples
long long critic_frag_offset();       // floats from the actor's W2^T fragments to the critic's
void launch_prep(hipStream_t s, const float *W2a, const float *W2c, int k2c, float4 *frag, const uint8_t *valid, long long n,
                 int *count);
void launch_sample(hipStream_t s, bool critic, const PassArgs &p);
void launch_wgrad(hipStream_t s, bool critic, const SampleRows &r, long long n_pad, long long slice_rows, int slices, float *part);

}  // namespace pt
}  // namespace mm
#endif
