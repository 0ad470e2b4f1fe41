// policy_bank_args.cpp -- the host side of include/mm_policy_bank.h under a host sanitizer: every argument check, through
// calls that are refused before anything is enqueued, and the grid-split arithmetic on the group layouts of the tests.  No
// kernel is launched and no device is needed; the pointers handed over are never dereferenced by the host code (it only tests
// them for NULL), so plain host arrays stand in for device memory.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/policy_bank_args.cpp \
//         marl-mass_amd/csrc/mm_policy_bank.hip -o policy_bank_args && ./policy_bank_args
//
// Prints the number of checks and exits 0 when every refused call returned MM_ERR_INVALID_ARG and every split kept its promises:
// an empty group has no workgroup, every other group at least one and never more than it has tile octets, the block prefix is
// consistent, and the grid is at most MM_BANK_MAX_GRID + K.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/mm_policy_bank.h"

static int checks = 0, failures = 0;

static void expect(bool ok, const char *what) {
  checks++;
  if (!ok) {
    failures++;
    std::fprintf(stderr, "FAILED: %s\n", what);
  }
}

struct Call {
  const float *obs;
  int64_t n;
  int32_t n_s;
  const MMMlpParams *bank;
  int32_t K;
  const int64_t *group_start;
  int32_t hidden, n_a;
  uint64_t *counter;
  int32_t *actions;
  float *logp;
};

static int32_t run(const Call &c) {
  return mm_policy_bank_act(c.obs, c.n, c.n_s, c.bank, c.K, c.group_start, c.hidden, c.n_a, 7, c.counter, c.actions, c.logp, nullptr);
}

static void check_split(const char *name, const std::vector<int64_t> &sizes) {
  const int K = (int)sizes.size();
  std::vector<int64_t> start(K + 1, 0);
  for (int k = 0; k < K; k++) start[k + 1] = start[k] + sizes[k];
  // exactly K + 1 entries, allocated on the heap: a read or a write past either table is the sanitizer's to report
  std::vector<int32_t> bs(K + 1, -1);
  expect(mm_policy_bank_grid(K, start.data(), bs.data()) == MM_OK, name);
  expect(bs[0] == 0, "the prefix starts at 0");
  long long cap_sum = 0;
  for (int k = 0; k < K; k++) {
    const long long tiles = (sizes[k] + MM_BANK_TILE - 1) / MM_BANK_TILE, cap = (tiles + MM_BANK_WAVES - 1) / MM_BANK_WAVES;
    const int blocks = bs[k + 1] - bs[k];
    cap_sum += cap;
    expect(blocks >= 0, "the prefix does not decrease");
    expect((blocks == 0) == (sizes[k] == 0), "an empty group has no workgroup, every other at least one");
    expect(blocks <= cap, "no workgroup without a tile");
  }
  expect(bs[K] >= 1 && bs[K] <= MM_BANK_MAX_GRID + K, "the grid is at most 256 + K");
  if (cap_sum <= MM_BANK_MAX_GRID) expect(bs[K] == cap_sum, "a small batch gets one tile per wave");
  else expect(bs[K] >= MM_BANK_MAX_GRID, "a large batch uses the whole budget");
}

int main() {
  // ---- the grid split: the five kinds of layout of tests/policy_bank_util.py, and the corners of the proportional branch
  for (int64_t n : {1, 32, 33, 257}) check_split("K = 1", {n});
  check_split("(1, 31, 33)", {1, 31, 33});
  check_split("(0, 40, 0, 24, 0)", {0, 40, 0, 24, 0});
  check_split("64 groups of 4", std::vector<int64_t>(64, 4));
  check_split("(65541, 7)", {65541, 7});
  check_split("64 groups of 8192", std::vector<int64_t>(64, 8192));
  {
    std::vector<int64_t> lopsided(64, 1);
    lopsided[63] = 1ll << 24;
    check_split("63 single agents beside 2^24", lopsided);
    lopsided[63] = 1ll << 40;  // products of tiles and workgroups beyond 2^32
    lopsided[0] = 1ll << 39;
    check_split("2^39, 62 single agents, 2^40", lopsided);
    std::vector<int64_t> ramp;
    for (int k = 0; k < 64; k++) ramp.push_back(k % 3 == 0 ? 0 : 1000 * (k + 1));
    check_split("a ramp with every third group empty", ramp);
  }
  int32_t bs3[4];
  const int64_t from_one[] = {1, 2, 3}, falling[] = {0, 5, 4}, fine[] = {0, 5, 9};
  expect(mm_policy_bank_grid(2, from_one, bs3) == MM_ERR_INVALID_ARG, "grid: group_start[0] != 0");
  expect(mm_policy_bank_grid(2, falling, bs3) == MM_ERR_INVALID_ARG, "grid: group_start decreases");
  expect(mm_policy_bank_grid(0, fine, bs3) == MM_ERR_INVALID_ARG, "grid: K 0");
  expect(mm_policy_bank_grid(MM_BANK_MAX_GROUPS + 1, fine, bs3) == MM_ERR_INVALID_ARG, "grid: K 65");
  expect(mm_policy_bank_grid(2, nullptr, bs3) == MM_ERR_INVALID_ARG, "grid: group_start NULL");
  expect(mm_policy_bank_grid(2, fine, nullptr) == MM_ERR_INVALID_ARG, "grid: block_start NULL");
  // ---- refused calls: a well-formed call, then one argument off at a time
  static float f[64];
  static int32_t a[64];
  static uint64_t ctr[1];
  const MMMlpParams w = {f, f, f, f, f, f};
  const int64_t start[] = {0, 1, 32, 65}, start0[] = {1, 1, 32, 65}, fall[] = {0, 40, 32, 65}, shortn[] = {0, 1, 32, 64},
                past[] = {0, 1, 32, 66}, neg[] = {0, 0, 0, -1}, zeros[] = {0, 0, 0, 0};
  const Call ok = {f, 65, 30, &w, 3, start, 128, 5, ctr, a, f};
  Call c;
#define REFUSED(what, change) c = ok; change; expect(run(c) == MM_ERR_INVALID_ARG, what)
  REFUSED("obs NULL", c.obs = nullptr);
  REFUSED("bank NULL", c.bank = nullptr);
  REFUSED("group_start NULL", c.group_start = nullptr);
  REFUSED("counter NULL", c.counter = nullptr);
  REFUSED("actions NULL", c.actions = nullptr);
  for (int j = 0; j < 6; j++) {
    MMMlpParams hollow = w;
    float **const field[6] = {&hollow.W1, &hollow.b1, &hollow.W2, &hollow.b2, &hollow.W3, &hollow.b3};
    *field[j] = nullptr;
    REFUSED("a NULL member base", c.bank = &hollow);
  }
  REFUSED("K 0", c.K = 0);
  REFUSED("K 65", c.K = MM_BANK_MAX_GROUPS + 1);  // (refused before group_start[65] would be read)
  REFUSED("hidden 512", c.hidden = 512);
  REFUSED("hidden 64", c.hidden = 64);
  REFUSED("n_s 0", c.n_s = 0);
  REFUSED("n_s 33", c.n_s = 33);
  REFUSED("n_a 0", c.n_a = 0);
  REFUSED("n_a 9", c.n_a = 9);
  REFUSED("n < 0", (c.n = -1, c.group_start = neg));
  REFUSED("group_start[0] != 0", c.group_start = start0);
  REFUSED("group_start decreases", c.group_start = fall);
  REFUSED("group_start ends short of n", c.group_start = shortn);
  REFUSED("group_start ends past n", c.group_start = past);
  c = ok; c.n = 0; c.group_start = zeros;
  expect(run(c) == MM_OK && ctr[0] == 0, "n == 0 is a no-op");
  c.logp = nullptr;
  expect(run(c) == MM_OK, "n == 0 without logp");
  std::printf("%d checks, %d failed\n", checks, failures);
  return failures ? 1 : 0;
}
