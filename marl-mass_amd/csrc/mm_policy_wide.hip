// mm_policy_wide.hip -- the reference's hidden-512 actor fused with the action sample (include/mm_policy_wide.h).
//
// marl/single_agent/Model_common.py:5-22 ActorNetwork at actor_hidden_size = 512 (the lateral_control = steer_vel .ini
// family), on f32-input MFMA in the transposed, one-wave-per-32-agents layout that mm_policy_mfma.h describes: an accumulator
// tile is directly the B operand of the next layer, activations never leave the register file.  What is new against
// policy_kernel is that neither fc2 (1 MiB) fits the LDS nor a whole layer (16 tiles = 256 registers per lane) fits the
// register file beside another one, so:
//
//   halves   fc2's 512 outputs are computed in two halves of 8 accumulator tiles (128 registers), which stay live.
//   chunks   per half, the 512-long reduction is walked in 16 chunks of 32 features.  Chunk c of h1 is produced where it is
//            consumed: ReLU of 16 MFMAs against W1[32 c .. 32 c + 31][:] (n_s padded to 32 with zeros), 16 registers that
//            are the B operands of the chunk's 8 x 16 fc2 MFMAs.  h1 is therefore computed once per half (2 x 256 MFMAs on
//            top of fc2's 4096).
//   slabs    chunk c of a half needs W2[256 half .. + 256][32 c .. + 32] (32 KB) and W1's 32 rows (4 KB): one slab, staged
//            by the whole workgroup for all of its waves, double-buffered, one barrier per chunk.  W2 in torch layout is
//            already A-fragment order in 16-byte pieces -- lane (i, h) needs W2[32 m + i][32 c + 8 g + 4 h .. + 3] for k-steps
//            4 g .. 4 g + 3 -- so a slab is a permutation of float4: global_load_dwordx4 along the rows (8 lanes per 128-byte
//            row piece) one per mfma4 early in the chunk, ds_write_b128 (lane index xor-swizzled, conflict-free) in its last
//            third, conflict-free ds_read_b128 one mfma4 ahead of its four MFMAs: see chunk().
//   heads    each finished half is folded tile by tile into the <= 8 head sums on the VALU (fc3's rows in LDS, 16 KB), then
//            one cross-half add, log-softmax (fp32) and the inverse-CDF sample (fp64) of mm_sample_actions, written by h = 0.
//
// Every sum is a fixed chain in a fixed order per row: a row's outputs do not depend on its tile, wave, workgroup or n.
#include "mm_policy_mfma.h"
#include "../../include/mm_policy_wide.h"

namespace mm {
namespace wide {
using namespace mfma;  // frag_row, mfma4, relu, max8, exp_shifted, persistent_grid

constexpr int kWide = 512;                          // hidden size
constexpr int kWaves = MM_POLICY_WIDE_WAVES;        // one wave per SIMD: the register file holds 8 accumulator tiles per wave
constexpr int kThreads = 64 * kWaves;
constexpr int kHalfTiles = 8;                       // output tiles of one half of fc2
constexpr int kChunks = kWide / 32;                 // 32-feature chunks of the reduction
constexpr int kSlabs = 2 * kChunks;                 // slabs of one trip: (half, chunk)
constexpr int kSlabPer = kHalfTiles * 4 * 64 / kThreads;  // float4 of a slab's W2 part per thread
constexpr uint32_t kDomain = 0x53414D50u;           // the sampler's Philox domain word (mm_sample_actions / mm_policy_act)
static_assert(MM_POLICY_WIDE_TILE == 32, "one MFMA tile of agents per wave");
static_assert(kSlabPer * kThreads == kHalfTiles * 4 * 64 && kThreads >= 256, "a slab divides evenly; W1's part needs 256 threads");
static_assert((kChunks & 1) == 0, "the slab's buffer is its index's parity in every half and trip");

// four consecutive k-steps' fragments as a native vector: its loads and stores are single instructions (dwordx4, b128) that
// the compiler keeps in registers and where they are written (HIP's float4 is copied with memcpy, which it forwards from the
// global load straight to the LDS write, behind the MFMAs)
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Slab {
  f32x4 w2[kHalfTiles][4][64];  // [out tile][k-step / 4][lane]: 32 KB
  f32x4 w1[4][64];              // [k-step / 4][lane]: 4 KB
};

MM_DEV f32x16 mfma4v(const f32x4 a, float b0, float b1, float b2, float b3, f32x16 acc) {
  return mfma4(make_float4(a.x, a.y, a.z, a.w), b0, b1, b2, b3, acc);
}

// a thread's part of a slab between its global loads and its LDS writes
struct Staged {
  f32x4 w2[kSlabPer];
  float w1[4];
};

// slab s = 16 half + chunk.  W2: thread t reads piece p = t & 7 (4 floats) of row t >> 3 of the half, consecutive lanes on
// consecutive 16 bytes.  W1: thread t < 256 gathers the four k-steps 4 q .. 4 q + 3 of lane l (q = t >> 6, l = t & 63).
MM_DEV void load_slab(Staged &st, const float *W1, const float *W2, int n_s, int s) {
  const int hf = s >> 4, c = s & 15;
  const unsigned tid = threadIdx.x;
#pragma unroll
  for (int u = 0; u < kSlabPer; u++) {
    const unsigned t = tid + u * kThreads, row = t >> 3, p = t & 7;
    st.w2[u] = *reinterpret_cast<const f32x4 *>(W2 + (256 * hf + row) * kWide + 32 * c + 4 * p);
  }
  if (kThreads == 256 || tid < 256) {
    const int l = tid & 63, q = tid >> 6;
    const float *row = W1 + (32 * c + (l & 31)) * n_s;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = frag_row(4 * q + u, l >> 5);
      st.w1[u] = row[k < n_s ? k : 0];  // always a load of the row (no branch here); store_slab zeroes the padding
    }
  }
}

// where lane (i, h) finds its fragment of k-step group g: the xor permutes within aligned blocks of 8 lanes, which leaves every
// 16-lane group of a ds_read_b128 on 16 different slots
MM_DEV int frag_lane(int lane, int g) { return lane ^ (2 * g + (lane >> 5)); }

// part 0 .. kStoreParts - 1 of the slab (every call site passes a constant), or all of it with part < 0
constexpr int kStoreParts = 3;
MM_DEV void store_slab(Slab &sl, const Staged &st, int n_s, int part = -1) {
  const unsigned tid = threadIdx.x;
#pragma unroll
  for (int u = 0; u < kSlabPer; u++) {
    if (part >= 0 && u * kStoreParts / kSlabPer != part) continue;
    const unsigned t = tid + u * kThreads, row = t >> 3, p = t & 7;
    // piece p = 2 g + h belongs to lane (row & 31, h).  The 8 lanes of a ds_write_b128 group hold the 8 pieces of one row: the
    // lane index is xor-ed with p, which puts them on 8 different 16-byte slots; frag_lane is the reader's side of it
    sl.w2[row >> 5][p >> 1][((row & 31) ^ p) + 32 * (p & 1)] = st.w2[u];
  }
  if ((part < 0 || part == kStoreParts - 1) && (kThreads == 256 || tid < 256)) {
    const int l = tid & 63, q = tid >> 6;
    f32x4 w;
#pragma unroll
    for (int u = 0; u < 4; u++) w[u] = frag_row(4 * q + u, l >> 5) < n_s ? st.w1[u] : 0.0f;
    sl.w1[q][l] = w;
  }
}

// One chunk of one half for a wave's tile: h1's 32 features of the chunk, then their contribution to the half's 8 accumulator
// tiles, out of slab `rd`; meanwhile the workgroup's next slab (index `next`) goes from global memory into `wr`.  rd and wr are
// two variables, not two elements of one array, so that the compiler knows the writes from the reads.
MM_DEV void chunk(const Slab &rd, Slab &wr, Staged &st, f32x16 (&acc)[kHalfTiles], const float (&xk)[16], const float *sB1c,
                  const float *W1, const float *W2, int n_s, int next, int lane, int h) {
  f32x16 a1;
#pragma unroll
  for (int r = 0; r < 16; r++) a1[r] = sB1c[frag_row(r, h)];
  f32x4 frag = rd.w1[0][lane];
  __builtin_amdgcn_sched_barrier(0);
  // One wave per SIMD has nobody to hide a latency behind, so the chunk is one pinned pipeline of 36 stages, a stage being a
  // fragment's four MFMAs (4 of fc1, 32 of fc2):
  //   every stage  reads the next stage's fragment first (the compiler alone reads each fragment into the one register
  //                quadruple right before its MFMAs and waits for it);
  //   kLoadAt ..   one global load of the next slab per stage, 8 + 4 of them;
  //   kStoreAt ..  the LDS writes of that slab in kStoreParts groups of three, kStoreGap stages apart and some 3000 MFMA cycles
  //                after their loads were issued; each group is fenced where it stands (hints alone let a write follow its
  //                load at once, and wait for it).  wr was last read in the chunk before this one, which every wave left
  //                through a barrier.
  // (sched_group_barrier: 0x8 MFMA, 0x20 VMEM read, 0x100 DS read.)
  constexpr int kStages = 4 + 4 * kHalfTiles, kLoadAt = 1, kLoads = kSlabPer + 4, kStoreAt = 24, kStoreGap = 3;
  static_assert(kLoadAt + kLoads <= kStoreAt - 8 && kStoreAt + kStoreGap * kStoreParts <= kStages, "loads, then stores, inside the chunk");
  load_slab(st, W1, W2, n_s, next);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const f32x4 nxt = q < 3 ? rd.w1[q + 1][lane] : rd.w2[0][0][frag_lane(lane, 0)];
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x8, 4, 0);
    if (q >= kLoadAt) __builtin_amdgcn_sched_group_barrier(0x20, 1, 0);
    a1 = mfma4v(frag, xk[4 * q + 0], xk[4 * q + 1], xk[4 * q + 2], xk[4 * q + 3], a1);
    frag = nxt;
  }
  const f32x16 h1 = relu(a1);  // features 32 c + frag_row(r, h): register r is the B operand of k-step r
#pragma unroll
  for (int f = 0; f < 4 * kHalfTiles; f++) {  // fragment f: k-steps 4 g .. 4 g + 3 of output tile m
    const int g = f / kHalfTiles, m = f % kHalfTiles, stage = 4 + f;
    if (stage >= kStoreAt && (stage - kStoreAt) % kStoreGap == 0 && (stage - kStoreAt) / kStoreGap < kStoreParts) {
      __builtin_amdgcn_sched_barrier(0);
      store_slab(wr, st, n_s, (stage - kStoreAt) / kStoreGap);
      __builtin_amdgcn_sched_barrier(0);
    }
    f32x4 nxt = frag;
    if (f + 1 < 4 * kHalfTiles) {
      nxt = rd.w2[(f + 1) % kHalfTiles][(f + 1) / kHalfTiles][frag_lane(lane, (f + 1) / kHalfTiles)];
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x8, 4, 0);
    if (stage < kLoadAt + kLoads) __builtin_amdgcn_sched_group_barrier(0x20, 1, 0);
    acc[m] = mfma4v(frag, h1[4 * g + 0], h1[4 * g + 1], h1[4 * g + 2], h1[4 * g + 3], acc[m]);
    frag = nxt;
  }
  __builtin_amdgcn_sched_barrier(0);
  __syncthreads();  // one barrier per chunk: wr is complete, and nobody reads rd any more
}

__global__ __launch_bounds__(kThreads) void policy_wide_kernel(const float *__restrict__ obs, long long n, int n_s,
                                                               const float *W1, const float *__restrict__ b1,
                                                               const float *W2, const float *__restrict__ b2,
                                                               const float *__restrict__ W3, const float *__restrict__ b3, int n_a,
                                                               uint64_t seed, const uint64_t *__restrict__ counter,
                                                               int32_t *__restrict__ actions, float *__restrict__ logp_out) {
  __shared__ Slab slab0, slab1;     // double buffer: 72 KB
  __shared__ float sW3[8][kWide];   // fc3's rows, zero past n_a: 16 KB
  __shared__ float sB1[kWide], sB2[kWide], sB3[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  for (int t = tid; t < 8 * kWide; t += kThreads) sW3[t / kWide][t % kWide] = (t / kWide) < n_a ? W3[t] : 0.0f;
  for (int t = tid; t < kWide; t += kThreads) { sB1[t] = b1[t]; sB2[t] = b2[t]; }
  if (tid < 8) sB3[tid] = tid < n_a ? b3[tid] : 0.0f;
  Staged st;
  load_slab(st, W1, W2, n_s, 0);
  store_slab(slab0, st, n_s);
  __syncthreads();
  const uint64_t ctr = *counter;
  const long long ntiles = (n + 31) / 32;
  // every wave of a workgroup makes the same trips (the slabs are staged by all of them); a wave past the last tile computes
  // on zeros and writes nothing
  for (long long base = (long long)blockIdx.x * kWaves; base < ntiles; base += (long long)gridDim.x * kWaves) {
    const long long ag = (base + wave) * 32 + j;
    const bool live = ag < n;
    float xk[16];  // B operand of layer 1: x[agent j][k(s, h)]
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const int k = frag_row(s, h);
      xk[s] = (live && k < n_s) ? obs[ag * n_s + k] : 0.0f;
    }
    float p[8];  // the head sums (before the cross-half add and the bias)
#pragma unroll
    for (int o = 0; o < 8; o++) p[o] = 0.0f;
#pragma unroll 1
    for (int hf = 0; hf < 2; hf++) {
      f32x16 acc[kHalfTiles];
#pragma unroll
      for (int m = 0; m < kHalfTiles; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[m][r] = sB2[256 * hf + 32 * m + frag_row(r, h)];
#pragma unroll 1
      for (int c = 0; c < kChunks; c += 2) {
        const int s = kChunks * hf + c;  // slab s is in buffer s & 1, and kChunks is even
        chunk(slab0, slab1, st, acc, xk, sB1 + 32 * c, W1, W2, n_s, s + 1, lane, h);
        chunk(slab1, slab0, st, acc, xk, sB1 + 32 * (c + 1), W1, W2, n_s, (s + 2) & (kSlabs - 1), lane, h);
      }
      // ---- layer 3, this half's share: ReLU and n_a x 16 FMAs per tile, tile by tile
#pragma unroll
      for (int m = 0; m < kHalfTiles; m++) {
        const f32x16 h2 = relu(acc[m]);
#pragma unroll
        for (int o = 0; o < 8; o++) {
          if (o < n_a) {
#pragma unroll
            for (int r = 0; r < 16; r++) p[o] = fmaf(h2[r], sW3[o][256 * hf + 32 * m + frag_row(r, h)], p[o]);
          }
        }
      }
    }
    // ---- log-softmax + sample (policy_kernel's tail)
    float logit[8];
#pragma unroll
    for (int o = 0; o < 8; o++) {
      const float t = p[o] + __shfl_xor(p[o], 32, 64);
      logit[o] = o < n_a ? t + sB3[o] : -INFINITY;
    }
    const float mx = max8(logit);
    float se = 0.0f;
#pragma unroll
    for (int o = 0; o < 8; o++) se += exp_shifted(logit[o], mx, o < n_a);
    const float lg = logf(se);  // (logit - mx) - log(sum), torch's order: the normaliser is not rounded at ulp(mx)
    if (live && h == 0) {
      double cdf[8], acc = 0;
#pragma unroll
      for (int o = 0; o < 8; o++) {
        const float lp = (logit[o] - mx) - lg;
        if (o < n_a) {
          if (logp_out) logp_out[ag * n_a + o] = lp;
          acc = acc + mmm_exp((double)lp);
          cdf[o] = acc;
        }
      }
      uint32_t w4[4];
      philox4x32((uint32_t)ag, (uint32_t)((uint64_t)ag >> 32), (uint32_t)ctr, (uint32_t)(ctr >> 32) ^ kDomain, (uint32_t)seed,
                 (uint32_t)(seed >> 32), w4);
      const double u = u53(w4[0], w4[1]);
      int a = 0;
#pragma unroll
      for (int o = 0; o < 8; o++)
        if (o < n_a) a += (cdf[o] / acc <= u) ? 1 : 0;  // searchsorted(cdf / cdf[-1], u, "right")
      actions[ag] = a < n_a - 1 ? a : n_a - 1;
    }
  }
}

__global__ void wide_counter_bump_kernel(uint64_t *counter) { *counter += 1; }

}  // namespace wide
}  // namespace mm

extern "C" int32_t mm_policy_wide_act(const float *obs, int64_t n, int32_t n_s, const float *W1, const float *b1, const float *W2,
                                      const float *b2, const float *W3, const float *b3, int32_t hidden, int32_t n_a, uint64_t seed,
                                      uint64_t *counter, int32_t *actions, float *logp, MMStream stream) {
  using namespace mm::wide;
  if (!obs || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !counter || !actions) return MM_ERR_INVALID_ARG;
  if (n < 0 || n_s < 1 || n_s > 32 || hidden != kWide || n_a < 1 || n_a > 8) return MM_ERR_INVALID_ARG;
  if ((uintptr_t)W2 % MM_POLICY_WIDE_W2_ALIGN != 0) return MM_ERR_INVALID_ARG;  // the slabs are 16-byte loads
  if (n == 0) return MM_OK;
  hipStream_t s = (hipStream_t)stream;
  const long long ntiles = (n + 31) / 32;
  static_assert(MM_POLICY_WIDE_MAX_GRID == 256, "persistent_grid launches one workgroup per CU");
  const unsigned grid = persistent_grid(ntiles, kWaves);
  hipLaunchKernelGGL(policy_wide_kernel, dim3(grid), dim3(kThreads), 0, s, obs, (long long)n, (int)n_s, W1, b1, W2, b2, W3, b3,
                     (int)n_a, seed, (const uint64_t *)counter, actions, logp);
  hipLaunchKernelGGL(wide_counter_bump_kernel, dim3(1), dim3(1), 0, s, counter);
  return hipGetLastError() == hipSuccess ? MM_OK : MM_ERR_DEVICE;
}
