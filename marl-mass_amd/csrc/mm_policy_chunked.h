// mm_policy_chunked.h -- how the entries of the hidden-128 training files reach prep, kernel A and kernel B, and what the chunked
// entries (mm_policy_chunked.hip) and the rank-sharded ones (mm_policy_sharded.hip) of all three families share (below).  The launch helpers are
// host-side only, defined next to the kernels they launch (mm_policy_gi_train.hip, mm_policy_train.hip) and used by the unchunked
// entries of those files as by the pass loops: every launch of prep, A and B is spelled once.  The pass loops add no __global__
// to those files and edit none, so their code objects stay as recorded (profiles/policy_gi_train, profiles/policy_train).  A
// helper only enqueues on the stream; the caller reads hipGetLastError.
#ifndef MM_POLICY_CHUNKED_H
#define MM_POLICY_CHUNKED_H
#include "mm_policy_mfma.h"  // and with it the two public headers
#include "mm_policy_wide_chunked.h"  // wt::, the same launch helpers for the hidden-512 networks (mm_policy_wide_train.hip)

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
bool zero_grads(hipStream_t s, const MMGiParams &g, int n_a);  // the n == 0 path: the twelve gradients; false: an enqueue failed

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
// ---- what the chunked entries (mm_policy_chunked.hip) and the rank-sharded ones (mm_policy_sharded.hip) share: the two hidden
// sizes of the separate networks as traits, the index maps of the finish kernels, the chunked scratch layout, the argument checks,
// the pass loops and the accumulate launch
namespace chunked {

typedef mfma::PartialBlock<5> PartGi;  // the shared network's partial block: 27 952 floats

static inline SampleRows rows_of(float *sc, const mfma::Layout &R) {
  SampleRows r = {sc + R.h1, sc + R.dz1, sc + R.h2, sc + R.dz2, sc + R.dh, sc + R.xs};
  return r;
}

// the partial blocks of a chunked scratch at hidden 128: the slices of the unchunked layout of `chunk` samples up to 1024 tiles,
// where the count grows with the size, and kMaxSlices above (a shorter last pass may cut more, never more than that)
static inline int narrow_blocks(const mfma::Layout &rows) { return rows.ntiles <= 2 * mfma::kMaxSlices ? rows.slices : mfma::kMaxSlices; }

// ---- the separate actor and critic at hidden 128 (mm_policy_train.hip) and 512 (mm_policy_wide_train.hip): what differs between
// the two, and nothing else.  Part: one slice's partial block, the same members in the same order at both sizes (kW2 [kHid][kPitch],
// kHd [16][kHid], kW1 [kHid][32], kb2, kbh, kb1).  kWideBit: what the size adds to a shard block's configuration word.  prep,
// bind (the scratch at sc -> network k's prepared fc2 operands and the rows of a pass), sample and wgrad forward to the launch
// helpers defined next to the kernels.
struct Pt128 {
  typedef pt::PassArgs PassArgs;
  typedef mfma::Layout Layout;
  typedef mfma::PartialBlock<4> Part;  // 26 896 floats
  static constexpr int kHid = mfma::kHidden, kPitch = mfma::kW2Pitch, kAlign = 16, kWideBit = 0;
  static Layout layout_of(long long n) { return pt::layout_of(n); }
  static int blocks(long long, const Layout &rows) { return narrow_blocks(rows); }
  static void prep(hipStream_t s, const float *W2a, const float *W2c, int k2c, float *sc, const Layout &R, const uint8_t *valid,
                   long long n) {
    pt::launch_prep(s, W2a, W2c, k2c, (float4 *)(sc + R.frag), valid, n, (int *)sc);
  }
  static void bind(PassArgs &p, float *sc, const Layout &R, int k) {
    p.frag = (const float4 *)(sc + R.frag + k * pt::critic_frag_offset());
    p.rows = rows_of(sc, R);
  }
  static void sample(hipStream_t s, bool critic, const PassArgs &p) { pt::launch_sample(s, critic, p); }
  static void wgrad(hipStream_t s, bool critic, const PassArgs &p, const Layout &P, float *part) {
    pt::launch_wgrad(s, critic, p.rows, P.n_pad, P.slice_rows, P.slices, part);
  }
};

struct Pt512 {
  typedef wt::PassArgs PassArgs;
  typedef wt::WideLayout Layout;
  typedef wt::Part Part;  // 304 144 floats
  static constexpr int kHid = wt::kWide, kPitch = wt::kCat, kAlign = MM_POLICY_WIDE_TRAIN_SCRATCH_ALIGN, kWideBit = 1 << 26;
  static Layout layout_of(long long n) { return wt::layout_of(n); }
  // the most slices ANY pass of at most `chunk` samples cuts, not the slices of a full pass (include/mm_policy_wide_train.h)
  static int blocks(long long chunk, const Layout &) { return (int)MM_POLICY_WIDE_TRAIN_CHUNKED_BLOCKS(chunk); }
  static void prep(hipStream_t s, const float *W2a, const float *W2c, int k2c, float *sc, const Layout &R, const uint8_t *valid,
                   long long n) {
    wt::launch_prep(s, W2a, W2c, k2c, sc + R.w2t, sc + R.w2p, valid, n, (int *)sc);
  }
  static void bind(PassArgs &p, float *sc, const Layout &R, int k) {
    p.w2t = sc + R.w2t + k * wt::kSquare;
    p.w2p = sc + R.w2p + k * wt::kSquare;
    const wt::WideRows rows = {sc + R.xs, sc + R.h1, sc + R.h2, sc + R.dz2, sc + R.dz1, sc + R.dh};
    p.rows = rows;
  }
  static void sample(hipStream_t s, bool critic, const PassArgs &p) { wt::launch_sample(s, critic, p); }
  static void wgrad(hipStream_t s, bool critic, const PassArgs &p, const Layout &P, float *part) {
    wt::launch_wgrad(s, critic, p.rows, P.n_pad, P.slice_rows, P.slices, part);
  }
};

constexpr int kCatGi = 160;
constexpr int kNFixedGi = 32 * 5 + 32 + 64 * 10 + 64 + 64 * 10 + 64 + mfma::kHidden * kCatGi + mfma::kHidden;  // everything before Wa

// the gradient elements of the shared network (the twelve tensors of MMGiParams in order) and of one separate network (six)
__host__ __device__ inline int gi_elems(int n_a) { return kNFixedGi + n_a * mfma::kHidden + n_a + mfma::kHidden + 1; }
template <class F>
inline int grad_elems(int n_s, int k2, int n_out) { return mfma::fold_elems(F::kHid, n_s, k2, n_out); }

// policy_gi_train_fold_kernel's index map (mm_policy_gi_train.hip): element t < gi_elems(n_a) of the gradients in torch layout ->
// where it is written; src: its slot of the PartialBlock<5> accumulator
MM_DEV float *gi_grad_slot(int t, int n_a, const MMGiParams &gr, int &src) {
  typedef PartGi P;
  constexpr int kHidden = mfma::kHidden;
  if (t < 160) { const int o = t / 5, k = t % 5; src = P::kW1 + o * 32 + 5 * k; return gr.W11 + t; }
  t -= 160;
  if (t < 32) { src = P::kb1 + t; return gr.b11 + t; }
  t -= 32;
  if (t < 640) { const int o = t / 10, k = t % 10; src = P::kW1 + (32 + o) * 32 + 5 * (k >> 1) + 1 + (k & 1); return gr.W12 + t; }
  t -= 640;
  if (t < 64) { src = P::kb1 + 32 + t; return gr.b12 + t; }
  t -= 64;
  if (t < 640) { const int o = t / 10, k = t % 10; src = P::kW1 + (96 + o) * 32 + 5 * (k >> 1) + 3 + (k & 1); return gr.W13 + t; }
  t -= 640;
  if (t < 64) { src = P::kb1 + 96 + t; return gr.b13 + t; }
  t -= 64;
  if (t < kHidden * kCatGi) { src = P::kW2 + t; return gr.W2 + t; }
  t -= kHidden * kCatGi;
  if (t < kHidden) { src = P::kb2 + t; return gr.b2 + t; }
  t -= kHidden;
  if (t < n_a * kHidden) { src = P::kHd + t; return gr.Wa + t; }
  t -= n_a * kHidden;
  if (t < n_a) { src = P::kbh + t; return gr.ba + t; }
  t -= n_a;
  if (t < kHidden) { src = P::kHd + 8 * kHidden + t; return gr.Wc + t; }
  src = P::kbh + 8;
  return gr.bc;
}

// The index map of the two unchunked fold kernels (policy_train_fold_kernel, policy_wide_fold_kernel) for a network with fc2 rows
// of k2 floats and n_out outputs: element t of its six gradients -> where it is written (nullptr past the last element); src: its
// slot of the F::Part accumulator
template <class F>
MM_DEV float *grad_slot(int t, int n_s, int k2, int n_out, const MMMlpParams &gr, int &src) {
  typedef typename F::Part P;
  constexpr int kHid = F::kHid;
  if (t < kHid * n_s) { const int o = t / n_s, k = t % n_s; src = P::kW1 + o * 32 + k; return gr.W1 + t; }
  t -= kHid * n_s;
  if (t < kHid) { src = P::kb1 + t; return gr.b1 + t; }
  t -= kHid;
  if (t < kHid * k2) { const int o = t / k2, k = t % k2; src = P::kW2 + o * F::kPitch + k; return gr.W2 + t; }
  t -= kHid * k2;
  if (t < kHid) { src = P::kb2 + t; return gr.b2 + t; }
  t -= kHid;
  if (t < n_out * kHid) { src = P::kHd + t; return gr.W3 + t; }
  t -= n_out * kHid;
  src = P::kbh + t;
  return t < n_out ? gr.b3 + t : nullptr;
}

// its inverse: whether grad_slot<F> reads slot `off` of the accumulator for any element of such a network
template <class F>
MM_DEV bool slot_is_read(int off, int n_s, int k2, int n_out) {
  typedef typename F::Part P;
  if (off < P::kHd) return off % F::kPitch < k2;
  if (off < P::kW1) return off - P::kHd < n_out * F::kHid;
  if (off < P::kb2) return (off - P::kW1) % 32 < n_s;
  if (off < P::kbh) return true;
  if (off < P::kb1) return off - P::kbh < n_out;
  return true;
}

// ---- host side
// The chunked scratch, offsets in floats: the header, the prepared fc2 operands and the per-sample rows as in the unchunked layout
// of `chunk` samples (Rows: mfma::Layout | wt::WideLayout); then the fp64 loss partials of all ceil(n / 32) tiles, two doubles per
// tile (the shared network's two heads interleaved | the actor's double[ntiles], then the critic's), `blocks` partial blocks for
// one pass, and `nets` fp64 accumulator blocks (the sharded entries accumulate into the caller's shard block and leave them unused).
template <class Rows>
struct ChunkLayout {
  Rows rows;  // the unchunked layout of `chunk` samples
  long long ntiles, lossp, part, acc, total;
  int blocks;
};

template <class Rows>
static inline ChunkLayout<Rows> chunk_layout(const Rows &rows, long long n, int blocks, int partial, int nets) {
  ChunkLayout<Rows> L;
  L.rows = rows;
  L.ntiles = (n + 31) / 32;
  L.blocks = blocks;
  L.lossp = rows.lossp;  // (where the unchunked layout's own loss partials start: the end of the rows)
  L.part = L.lossp + 2 * 2 * L.ntiles;
  L.acc = L.part + (long long)blocks * partial;
  L.total = L.acc + 2ll * nets * partial;
  return L;
}

// the separate networks' (at 512, total * 4 == MM_POLICY_WIDE_TRAIN_CHUNKED_BYTES(n, chunk): tests/test_wide_chunked_host.py)
template <class F>
static inline ChunkLayout<typename F::Layout> chunk_layout_of(long long n, long long chunk) {
  static_assert(F::Part::kSize % 2 == 0, "the accumulators follow the partial blocks 8-byte aligned");
  const typename F::Layout rows = F::layout_of(chunk);
  return chunk_layout(rows, n, F::blocks(chunk, rows), F::Part::kSize, 2);
}

// acc[off] += the `slices` partial blocks of `size` floats at part, in workgroup order, fp64 (train_chunked_accumulate_kernel)
void accumulate(hipStream_t s, const float *part, int slices, int size, double *acc);

// one separate network of a call (NULL w: not given) and its per-sample outputs: logp_taken, ratio | value, unused
struct Net {
  const MMMlpParams *w;
  float *out0, *out1;
};

// What the chunked and the partial entry of a family refuse alike, on the whole batch's PassArgs (n the whole batch, the
// pointers at sample 0): the weights, the shape limits, critic_loss, clip_param, chunk, diagnostics without their network and,
// when n > 0, the per-sample inputs, adv_sums against advantages, and the scratch: its pointer, alignment and size, and that the
// two pass sizes there are, chunk and the last pass's, fit the rows and cut no more slices than the partial blocks hold.
// Enqueues nothing.  L: the scratch layout when n > 0.
bool gi_args_ok(const gi_train::PassArgs &batch, int32_t n_s, int32_t hidden, int32_t critic_loss, int64_t chunk, const void *scratch,
                uint64_t scratch_bytes, ChunkLayout<mfma::Layout> &L);
template <class F>
bool args_ok(const typename F::PassArgs &batch, const Net (&net)[2], int32_t hidden, int32_t critic_loss, int64_t chunk,
             const void *scratch, uint64_t scratch_bytes, ChunkLayout<typename F::Layout> &L);

// The passes of a batch of n > 0 samples that the checks above let through: prep once over the whole batch (its count of valid
// samples goes to the scratch header, the int at sc, which the caller has zeroed), then per pass of `chunk` samples kernel A
// (scaled by batch.count), kernel B and accumulate through the rows of the scratch at sc, the per-sample pointers of a copy of
// `batch` shifted on the host.  The separate networks take turns within a pass, the actor first; the critic's accumulator follows
// the actor's (acc + F::Part::kSize).
void gi_passes(hipStream_t s, const gi_train::PassArgs &batch, long long chunk, const ChunkLayout<mfma::Layout> &L, float *sc,
               double *acc);
template <class F>
void passes(hipStream_t s, const typename F::PassArgs &batch, const Net (&net)[2], long long chunk,
            const ChunkLayout<typename F::Layout> &L, float *sc, double *acc);

// (both templates are defined in mm_policy_chunked.hip and instantiated there for Pt128 and Pt512)

}  // namespace chunked
}  // namespace mm
#endif
