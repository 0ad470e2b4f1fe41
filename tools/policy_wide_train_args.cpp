// policy_wide_train_args.cpp -- the host side of include/mm_policy_wide_train.h under a host sanitizer: the scratch
// arithmetic and every argument check, through calls that are refused before anything is enqueued.  No kernel is launched and
// no device is needed; the pointers handed over are never dereferenced by the host code (it only tests them for NULL and
// alignment), so plain host arrays stand in for device memory.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/policy_wide_train_args.cpp \
//         marl-mass_amd/csrc/mm_policy_wide_train.hip -o policy_wide_train_args && ./policy_wide_train_args
//
// Prints the number of checks and exits 0 when every refused call returned MM_ERR_INVALID_ARG and the size query matched the
// header's stated sum.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../include/mm_policy_wide_train.h"

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
  int64_t obs_stride, n;
  int32_t n_s;
  const int32_t *actions;
  const float *returns, *old_logp;
  const MMMlpParams *actor, *critic;
  int32_t hidden, n_a;
  float clip;
  int32_t critic_loss;
  const float *adv_sums, *advantages;
  const MMMlpParams *ga, *gc;
  float *loss, *logp, *value, *ratio;
  void *scratch;
  uint64_t scratch_bytes;
};

static int32_t run(const Call &c) {
  return mm_policy_wide_train(c.obs, c.obs_stride, c.n, c.n_s, c.actions, 1, c.returns, 1, c.old_logp, nullptr, c.actor, c.critic,
                              c.hidden, c.n_a, c.clip, c.critic_loss, c.adv_sums, c.advantages, c.ga, c.gc, c.loss, c.logp, c.value,
                              c.ratio, c.scratch, c.scratch_bytes, nullptr);
}

static uint64_t stated(int64_t n) {
  const int64_t tiles = (n + MM_POLICY_WIDE_TRAIN_TILE - 1) / MM_POLICY_WIDE_TRAIN_TILE;
  int64_t per = (tiles + MM_POLICY_WIDE_TRAIN_MAX_SLICES - 1) / MM_POLICY_WIDE_TRAIN_MAX_SLICES;
  if (per < MM_POLICY_WIDE_TRAIN_MIN_SLICE_TILES) per = MM_POLICY_WIDE_TRAIN_MIN_SLICE_TILES;
  int64_t slices = (tiles + per - 1) / per;
  if (slices < 1) slices = 1;
  return (uint64_t)MM_POLICY_WIDE_TRAIN_FIXED_BYTES + (uint64_t)tiles * MM_POLICY_WIDE_TRAIN_TILE * MM_POLICY_WIDE_TRAIN_ROW_BYTES +
         8u * (uint64_t)tiles + (uint64_t)slices * MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES;
}

int main() {
  // ---- the size query
  uint64_t prev = 0;
  const int64_t sizes[] = {0, 1, 31, 32, 33, 1000, 65637, 524288, 2147483647LL};
  for (int64_t n : sizes) {
    uint64_t b = 0;
    expect(mm_policy_wide_train_scratch_bytes(n, &b) == MM_OK && b == stated(n) && b >= prev && b > 0, "scratch bytes are the header's sum");
    prev = b;
  }
  uint64_t b = 0;
  expect(mm_policy_wide_train_scratch_bytes(-1, &b) == MM_ERR_INVALID_ARG, "n < 0");
  expect(mm_policy_wide_train_scratch_bytes(64, nullptr) == MM_ERR_INVALID_ARG, "bytes NULL");
  // ---- refused calls: a well-formed call, then one argument off at a time
  static float f[64];
  static int32_t a[64];
  alignas(16) static unsigned char arena[64];
  MMMlpParams w = {f, f, f, f, f, f}, hollow = {f, f, f, f, f, nullptr};
  uint64_t need = 0;
  mm_policy_wide_train_scratch_bytes(500, &need);
  const Call ok = {f, 30, 500, 30, a, f, f, &w, &w, 512, 5, 0.2f, MM_PT_CRITIC_MSE, nullptr, f, &w, &w, f, nullptr, nullptr, nullptr,
                   arena, need};
  Call c;
#define REFUSED(what, change) c = ok; change; expect(run(c) == MM_ERR_INVALID_ARG, what)
  REFUSED("hidden 128", c.hidden = 128);
  REFUSED("hidden 256", c.hidden = 256);
  REFUSED("scratch NULL", c.scratch = nullptr);
  REFUSED("scratch one byte short", c.scratch_bytes = need - 1);
  REFUSED("scratch misaligned", c.scratch = arena + 4);
  REFUSED("neither form of the advantages", c.advantages = nullptr);
  REFUSED("both forms of the advantages", c.adv_sums = f);
  REFUSED("n_s 24", c.n_s = 24);
  REFUSED("n_s 33", c.n_s = 33);
  REFUSED("obs_stride < n_s", c.obs_stride = 29);
  REFUSED("clip < 0", c.clip = -0.1f);
  REFUSED("clip NaN", c.clip = __builtin_nanf(""));
  REFUSED("n_a 0", c.n_a = 0);
  REFUSED("n_a 9", c.n_a = 9);
  REFUSED("critic_loss 2", c.critic_loss = 2);
  REFUSED("no network", (c.actor = c.critic = c.ga = c.gc = nullptr));
  REFUSED("actor without gradients", c.ga = nullptr);
  REFUSED("gradients without critic", c.critic = nullptr);
  REFUSED("loss NULL", c.loss = nullptr);
  REFUSED("n < 0", c.n = -1);
  REFUSED("n > 2^31 - 1", c.n = 2147483648LL);
  REFUSED("a NULL pointer among the six", c.actor = &hollow);
  REFUSED("obs NULL", c.obs = nullptr);
  REFUSED("actions NULL", c.actions = nullptr);
  REFUSED("old_logp NULL", c.old_logp = nullptr);
  REFUSED("returns NULL", c.returns = nullptr);
  REFUSED("logp_taken without the actor", (c.actor = c.ga = nullptr, c.advantages = nullptr, c.logp = f));
  REFUSED("value without the critic", (c.critic = c.gc = nullptr, c.value = f));
  // ---- the evaluation
  expect(mm_policy_wide_eval(f, 30, 500, 30, a, 1, nullptr, &w, nullptr, 128, 5, f, nullptr, nullptr) == MM_ERR_INVALID_ARG, "eval hidden 128");
  expect(mm_policy_wide_eval(f, 30, 500, 30, a, 1, nullptr, &w, nullptr, 512, 5, nullptr, nullptr, nullptr) == MM_ERR_INVALID_ARG, "eval actor without output");
  expect(mm_policy_wide_eval(f, 30, 500, 30, a, 1, nullptr, nullptr, nullptr, 512, 5, f, nullptr, nullptr) == MM_ERR_INVALID_ARG, "eval no network");
  expect(mm_policy_wide_eval(f, 30, 500, 30, a, 1, nullptr, nullptr, &w, 512, 5, f, nullptr, nullptr) == MM_ERR_INVALID_ARG, "eval output without network");
  expect(mm_policy_wide_eval(f, 29, 500, 30, a, 1, nullptr, &w, nullptr, 512, 5, f, nullptr, nullptr) == MM_ERR_INVALID_ARG, "eval stride");
  expect(mm_policy_wide_eval(nullptr, 30, 0, 30, nullptr, 1, nullptr, &w, nullptr, 512, 5, nullptr, nullptr, nullptr) == MM_OK, "eval n == 0 is a no-op");
  std::printf("%d checks, %d failed\n", checks, failures);
  return failures ? 1 : 0;
}
