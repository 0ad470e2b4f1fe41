// mm_policy_bank_tables.h -- what the two training halves of the policy bank share (mm_policy_bank_train.hip: K actor / critic pairs,
// mm_policy_gi_bank_train.hip: K shared actor-critics): the group tables of a call and their lookups, the per-tile statistics and
// their fold per group, and the host-side plan that checks rows / row_len / K / col_start and fills the tables.  The statistics'
// bodies are force-inlined into a __global__ of each file, so each object keeps its own kernels.
#ifndef MM_POLICY_BANK_TABLES_H
#define MM_POLICY_BANK_TABLES_H
#include "mm_policy_mfma.h"
#include "../../include/mm_policy_bank.h"  // MM_BANK_MAX_GROUPS, mm_policy_bank_grid

namespace mm {
namespace bank_train {

constexpr int kG = MM_BANK_MAX_GROUPS;

// The group tables of a call; entries past K repeat the last one.
struct Tables {
  int col_start[kG + 1];    // member k owns columns [col_start[k], col_start[k + 1]) of every row
  int tile_start[kG + 1];   // prefix of the groups' 32-sample tiles: scratch rows of group k start at 32 tile_start[k]
  int slice_start[kG + 1];  // prefix of the groups' kernel-B slices = partial blocks
  int block_start[kG + 1];  // prefix of kernel A's workgroups
  int rows, row_len;
};

MM_DEV int group_of(const int (&start)[kG + 1], int b) {
  int g = 0;
#pragma unroll
  for (int k = 1; k < kG; k++) g += start[k] <= b ? 1 : 0;
  return g;
}

// member-local sample i of a group of width w starting at column c0 -> the batch's sample index
MM_DEV unsigned sample_of(unsigned i, unsigned w, unsigned c0, unsigned row_len) {
  const unsigned r = i / w;
  return r * row_len + c0 + (i - r * w);
}

struct StatArgs {
  const uint8_t *valid;
  const float *advantages, *target_value, *returns;
  long long ret_stride;
  int sums;  // reference form: S+ / S- are wanted
  double *stats;
};

// ---- stats: one wave per tile, lanes 0..31 one sample each (a 256-thread workgroup)
MM_DEV void stats_tiles(const StatArgs &p, const Tables &tb, int total_tiles) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = blockIdx.x * 4 + wave; t < total_tiles; t += gridDim.x * 4) {
    const int g = group_of(tb.tile_start, t);
    const unsigned c0 = tb.col_start[g], w = tb.col_start[g + 1] - c0;
    const long long ng = (long long)w * tb.rows;
    const long long local = (long long)(t - tb.tile_start[g]) * 32 + lane;
    double cnt = 0.0, sp = 0.0, sn = 0.0;
    if (lane < 32 && local < ng) {
      const unsigned gj = sample_of((unsigned)local, w, c0, (unsigned)tb.row_len);
      if (!p.valid || p.valid[gj] != 0) {
        cnt = 1.0;
        if (p.sums) {
          const float adv = p.advantages ? p.advantages[gj] : p.returns[gj * p.ret_stride] - p.target_value[gj];
          if (adv >= 0.0f) sp = (double)adv;
          else if (adv < 0.0f) sn = (double)adv;
        }
      }
    }
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) {
      cnt += __shfl_xor(cnt, o, 64);
      sp += __shfl_xor(sp, o, 64);
      sn += __shfl_xor(sn, o, 64);
    }
    if (lane == 0) {
      p.stats[3ll * t + 0] = cnt;
      p.stats[3ll * t + 1] = sp;
      p.stats[3ll * t + 2] = sn;
    }
  }
}

// ---- stats fold: workgroup k (256 threads) folds group k's tiles in loss_tree's fixed tree into B_k and the float S+_k, S-_k
MM_DEV void stats_fold(const double *__restrict__ stats, const Tables &tb, int *__restrict__ count, float *__restrict__ sums,
                       float *__restrict__ sums_out) {
  __shared__ double s[3][256];
  const int k = blockIdx.x;
  mfma::loss_tree<3>(stats + 3ll * tb.tile_start[k], tb.tile_start[k + 1] - tb.tile_start[k], s);
  if (threadIdx.x == 0) {
    count[k] = (int)s[0][0];
    sums[2 * k] = (float)s[1][0];
    sums[2 * k + 1] = (float)s[2][0];
    if (sums_out) {
      sums_out[2 * k] = (float)s[1][0];
      sums_out[2 * k + 1] = (float)s[2][0];
    }
  }
}

// ---- host side
struct Plan {
  Tables tb;
  long long total_tiles, total_slices, cap_slices;  // cap_slices: the partial blocks the scratch query reserves
  long long n;
};

// checks rows / row_len / K / col_start and fills the tables; false: refused
static bool plan(int64_t rows, int64_t row_len, int32_t K, const int64_t *col_start, bool with_grid, Plan &P) {
  using mfma::kMaxSlices;
  using mfma::tiles_per_slice;
  if (rows < 0 || row_len < 0 || !col_start || K < 1 || K > kG || col_start[0] != 0) return false;
  for (int k = 0; k < K; k++)
    if (col_start[k + 1] < col_start[k]) return false;
  if (col_start[K] != row_len) return false;
  if (row_len > 0 && rows > 0x7FFFFFFFll / row_len) return false;
  P.n = rows * row_len;
  int64_t size_start[kG + 1];
  Tables &tb = P.tb;
  tb.rows = (int)rows; tb.row_len = (int)row_len;
  tb.tile_start[0] = tb.slice_start[0] = 0;
  size_start[0] = 0;
  P.cap_slices = 0;
  for (int k = 0; k < K; k++) {
    const long long nk = (col_start[k + 1] - col_start[k]) * rows, nt = (nk + 31) / 32;
    const long long per = tiles_per_slice(nt);
    const long long cap = (nt + 1) / 2 < kMaxSlices ? (nt + 1) / 2 : kMaxSlices;
    tb.col_start[k] = (int)col_start[k];
    tb.tile_start[k + 1] = tb.tile_start[k] + (int)nt;
    tb.slice_start[k + 1] = tb.slice_start[k] + (int)((nt + per - 1) / per);
    size_start[k + 1] = size_start[k] + nk;
    P.cap_slices += cap;
  }
  for (int k = K; k <= kG; k++) {
    tb.col_start[k] = (int)row_len;
    tb.tile_start[k] = tb.tile_start[K];
    tb.slice_start[k] = tb.slice_start[K];
  }
  P.total_tiles = tb.tile_start[K];
  P.total_slices = tb.slice_start[K];
  for (int k = 0; k <= kG; k++) tb.block_start[k] = 0;
  if (with_grid && P.n > 0) {
    if (mm_policy_bank_grid(K, size_start, tb.block_start) != MM_OK) return false;
    for (int k = K + 1; k <= kG; k++) tb.block_start[k] = tb.block_start[K];
  }
  return true;
}

}  // namespace bank_train
}  // namespace mm
#endif
