// policy_bank_train_args.cpp -- the host side of include/mm_policy_bank_train.h and of mm_opt_step_bank (include/mm_opt_step.h)
// under a host sanitizer: every argument check of mm_policy_bank_eval, mm_policy_bank_train, mm_opt_step_bank and of the scratch
// query, through calls that are refused before anything is enqueued, and the query's arithmetic: it equals the header's formula and
// it never shrinks when a width grows.  No kernel is launched and no device is needed; the pointers handed over are never
// dereferenced by the host code (it only tests them for NULL and alignment), so plain host arrays stand in for device memory.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/policy_bank_train_args.cpp marl-mass_amd/csrc/mm_policy_bank_train.hip \
//         marl-mass_amd/csrc/mm_policy_bank.hip marl-mass_amd/csrc/mm_opt_step_bank.hip -o policy_bank_train_args \
//         && ./policy_bank_train_args
//
// Prints the number of checks and exits 0 when every refused call returned MM_ERR_INVALID_ARG and the query kept its promises.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/mm_opt_step.h"
#include "../include/mm_policy_bank_train.h"

// mm_opt_step_bank reports its refusals through the library's error slot (marl-mass_amd/csrc/mm_handle.h); stand-alone, here
static char last_error[256];
__attribute__((visibility("hidden"))) void mm_set_thread_error(const char *text) { std::snprintf(last_error, sizeof last_error, "%s", text); }

static int checks = 0, failures = 0;

static void expect(bool ok, const char *what) {
  checks++;
  if (!ok) {
    failures++;
    std::fprintf(stderr, "FAILED: %s\n", what);
  }
}

static std::vector<int64_t> prefix(const std::vector<int64_t> &w) {
  std::vector<int64_t> c(w.size() + 1, 0);  // exactly K + 1 entries on the heap: a read past the table is the sanitizer's to report
  for (size_t k = 0; k < w.size(); k++) c[k + 1] = c[k] + w[k];
  return c;
}

static uint64_t query(int64_t rows, const std::vector<int64_t> &w) {
  const std::vector<int64_t> c = prefix(w);
  uint64_t b = ~0ull;
  expect(mm_policy_bank_train_scratch_bytes(rows, c.back(), (int32_t)w.size(), c.data(), &b) == MM_OK, "the query accepts a layout");
  return b;
}

static uint64_t formula(int64_t rows, const std::vector<int64_t> &w) {
  uint64_t b = MM_PBT_HEADER_BYTES + (uint64_t)w.size() * MM_PBT_MEMBER_BYTES;
  for (int64_t wk : w) {
    const uint64_t t = (uint64_t)(rows * wk + 31) / 32, cap = (t + 1) / 2 < 512 ? (t + 1) / 2 : 512;
    b += 32 * t * MM_PBT_SAMPLE_BYTES + t * MM_PBT_TILE_BYTES + cap * MM_PBT_PARTIAL_BYTES;
  }
  return b;
}

struct Train {
  const float *obs;
  int64_t obs_stride, rows, row_len;
  int32_t n_s;
  const int32_t *actions;
  int64_t act_stride;
  const float *returns;
  int64_t ret_stride;
  const float *old_logp;
  const uint8_t *valid;
  const MMMlpParams *actors, *critics;
  int32_t K;
  const int64_t *col_start;
  int32_t hidden, n_a;
  float clip;
  int32_t critic_loss, form;
  const float *advantages, *target_value;
  const MMMlpParams *ga, *gc;
  float *loss, *adv_sums, *logp, *value, *ratio;
  void *scratch;
  uint64_t scratch_bytes;
};

static int32_t train(const Train &c) {
  return mm_policy_bank_train(c.obs, c.obs_stride, c.rows, c.row_len, c.n_s, c.actions, c.act_stride, c.returns, c.ret_stride, c.old_logp,
                              c.valid, c.actors, c.critics, c.K, c.col_start, c.hidden, c.n_a, c.clip, c.critic_loss, c.form,
                              c.advantages, c.target_value, c.ga, c.gc, c.loss, c.adv_sums, c.logp, c.value, c.ratio, c.scratch,
                              c.scratch_bytes, nullptr);
}

static int32_t eval(const Train &c) {
  return mm_policy_bank_eval(c.obs, c.obs_stride, c.rows, c.row_len, c.n_s, c.actions, c.act_stride, c.valid, c.actors, c.critics, c.K,
                             c.col_start, c.hidden, c.n_a, c.logp, c.value, nullptr);
}

int main() {
  // ---- the query: the header's formula on the layouts of the tests, and monotonic growth in every width
  const std::vector<std::pair<int64_t, std::vector<int64_t>>> layouts = {
      {7, {0, 5, 1, 17}}, {3, {64, 32}}, {41, {800, 1}}, {2, std::vector<int64_t>(64, 1)}, {5, {13}}, {0, {3, 4}}, {9, {0, 0}}};
  for (const auto &l : layouts) expect(query(l.first, l.second) == formula(l.first, l.second), "the query is the header's formula");
  for (const auto &l : layouts) {
    if (l.first == 0) continue;
    for (size_t k = 0; k < l.second.size(); k++) {
      std::vector<int64_t> w = l.second;
      uint64_t last = query(l.first, w);
      for (int64_t extra : {1, 1, 30, 1, 1, 700, 67, 1, 16384, 1 << 20}) {  // cumulative: across tile edges and the 1 024-tile edge
        w[k] += extra;
        const uint64_t now = query(l.first, w);
        expect(now >= last, "the query does not shrink when a width grows");
        last = now;
      }
    }
  }
  {
    uint64_t last = 0;
    for (int64_t n = 32 * 1000; n <= 32 * 1100; n += 8) {  // one group, step by step across 1 024 -> 1 025 tiles
      const uint64_t now = query(1, {n});
      expect(now >= last, "the query does not shrink across the slicing's edge");
      last = now;
    }
  }
  uint64_t bytes = 0;
  const int64_t fine[] = {0, 2, 5}, from_one[] = {1, 2, 5}, falling[] = {0, 3, 2}, shortn[] = {0, 2, 4}, huge[] = {0, 1ll << 31};
  expect(mm_policy_bank_train_scratch_bytes(2, 5, 2, fine, nullptr) == MM_ERR_INVALID_ARG, "query: bytes NULL");
  expect(mm_policy_bank_train_scratch_bytes(2, 5, 2, nullptr, &bytes) == MM_ERR_INVALID_ARG, "query: col_start NULL");
  expect(mm_policy_bank_train_scratch_bytes(-1, 5, 2, fine, &bytes) == MM_ERR_INVALID_ARG, "query: rows < 0");
  expect(mm_policy_bank_train_scratch_bytes(2, 5, 0, fine, &bytes) == MM_ERR_INVALID_ARG, "query: K 0");
  expect(mm_policy_bank_train_scratch_bytes(2, 5, MM_BANK_MAX_GROUPS + 1, fine, &bytes) == MM_ERR_INVALID_ARG, "query: K 65");
  expect(mm_policy_bank_train_scratch_bytes(2, 5, 2, from_one, &bytes) == MM_ERR_INVALID_ARG, "query: col_start[0] != 0");
  expect(mm_policy_bank_train_scratch_bytes(2, 5, 2, falling, &bytes) == MM_ERR_INVALID_ARG, "query: col_start decreases");
  expect(mm_policy_bank_train_scratch_bytes(2, 5, 2, shortn, &bytes) == MM_ERR_INVALID_ARG, "query: col_start ends short of row_len");
  expect(mm_policy_bank_train_scratch_bytes(1, 1ll << 31, 1, huge, &bytes) == MM_ERR_INVALID_ARG, "query: n > 2^31 - 1");
  expect(mm_policy_bank_train_scratch_bytes(1ll << 20, 1ll << 12, 1, huge, &bytes) == MM_ERR_INVALID_ARG, "query: rows * row_len > 2^31 - 1");
  // ---- refused calls of the two launches' entries: a well-formed call, then one argument off at a time
  alignas(16) static float f[64];
  static int32_t a[64];
  static uint8_t v[64];
  const MMMlpParams w = {f, f, f, f, f, f};
  expect(mm_policy_bank_train_scratch_bytes(2, 5, 2, fine, &bytes) == MM_OK, "query: the well-formed layout");
  const Train ok = {f, 30, 2, 5, 30, a, 1, f, 1, f, v, &w, &w, 2, fine, 128, 5, 0.2f, MM_PT_CRITIC_MSE, MM_PT_FORM_REFERENCE,
                    nullptr, f, &w, &w, f, f, f, f, f, f, bytes};
  Train c;
#define REFUSED(call, what, change) c = ok; change; expect(call(c) == MM_ERR_INVALID_ARG, what)
  for (int e = 0; e < 2; e++) {
    auto call = e ? eval : train;
    REFUSED(call, "no network", (c.actors = c.critics = nullptr, c.ga = c.gc = nullptr, c.logp = c.value = c.ratio = nullptr));
    REFUSED(call, "obs NULL", c.obs = nullptr);
    REFUSED(call, "actions NULL", c.actions = nullptr);
    REFUSED(call, "obs_stride < n_s", c.obs_stride = 29);
    REFUSED(call, "n_s 24", c.n_s = 24);
    REFUSED(call, "n_s 33", (c.n_s = 33, c.obs_stride = 33));
    REFUSED(call, "hidden 512", c.hidden = 512);
    REFUSED(call, "n_a 0", c.n_a = 0);
    REFUSED(call, "n_a 9", c.n_a = 9);
    REFUSED(call, "K 0", c.K = 0);
    REFUSED(call, "K 65", c.K = MM_BANK_MAX_GROUPS + 1);  // (refused before col_start[65] would be read)
    REFUSED(call, "col_start NULL", c.col_start = nullptr);
    REFUSED(call, "col_start[0] != 0", c.col_start = from_one);
    REFUSED(call, "col_start decreases", c.col_start = falling);
    REFUSED(call, "col_start ends short of row_len", c.col_start = shortn);
    REFUSED(call, "rows < 0", c.rows = -1);
    REFUSED(call, "n > 2^31 - 1", c.rows = 1ll << 30);
    for (int j = 0; j < 6; j++) {
      MMMlpParams hollow = w;
      float **const field[6] = {&hollow.W1, &hollow.b1, &hollow.W2, &hollow.b2, &hollow.W3, &hollow.b3};
      *field[j] = nullptr;
      REFUSED(call, "a NULL actor base", c.actors = &hollow);
      REFUSED(call, "a NULL critic base", c.critics = &hollow);
    }
  }
  REFUSED(eval, "eval: actors without logp_taken", c.logp = nullptr);
  REFUSED(eval, "eval: critics without value", c.value = nullptr);
  REFUSED(eval, "eval: logp_taken without actors", c.actors = nullptr);
  REFUSED(eval, "eval: value without critics", c.critics = nullptr);
  REFUSED(train, "loss NULL", c.loss = nullptr);
  REFUSED(train, "actors without gradients", c.ga = nullptr);
  REFUSED(train, "critics without gradients", c.gc = nullptr);
  REFUSED(train, "gradients without actors", (c.actors = nullptr, c.logp = c.ratio = nullptr, c.target_value = nullptr));
  REFUSED(train, "gradients without critics", (c.critics = nullptr, c.value = nullptr));
  for (int j = 0; j < 6; j++) {
    MMMlpParams hollow = w;
    float **const field[6] = {&hollow.W1, &hollow.b1, &hollow.W2, &hollow.b2, &hollow.W3, &hollow.b3};
    *field[j] = nullptr;
    REFUSED(train, "a NULL actor gradient", c.ga = &hollow);
    REFUSED(train, "a NULL critic gradient", c.gc = &hollow);
  }
  REFUSED(train, "critic_loss 2", c.critic_loss = 2);
  REFUSED(train, "form 2", c.form = 2);
  REFUSED(train, "form -1", c.form = -1);
  REFUSED(train, "clip_param < 0", c.clip = -0.1f);
  REFUSED(train, "clip_param NaN", c.clip = std::strtof("nan", nullptr));
  REFUSED(train, "neither advantages nor target_value", c.target_value = nullptr);
  REFUSED(train, "both advantages and target_value", c.advantages = f);
  REFUSED(train, "old_logp NULL with actors", c.old_logp = nullptr);
  REFUSED(train, "returns NULL with critics", c.returns = nullptr);
  REFUSED(train, "returns NULL with target_value", (c.returns = nullptr, c.critics = nullptr, c.gc = nullptr, c.value = nullptr));
  REFUSED(train, "logp_taken without actors", (c.actors = nullptr, c.ga = nullptr, c.ratio = nullptr, c.target_value = nullptr));
  REFUSED(train, "ratio without actors", (c.actors = nullptr, c.ga = nullptr, c.logp = nullptr, c.target_value = nullptr));
  REFUSED(train, "value without critics", (c.critics = nullptr, c.gc = nullptr));
  REFUSED(train, "scratch NULL", c.scratch = nullptr);
  REFUSED(train, "scratch misaligned", c.scratch = (char *)f + 4);
  REFUSED(train, "scratch one byte short", c.scratch_bytes = bytes - 1);
  // ---- mm_opt_step_bank
  MMOptGroup g;
  std::memset(&g, 0, sizeof g);
  g.algo = MM_OPT_ADAM; g.n_tensors = 2;
  for (int i = 0; i < 2; i++) { g.count[i] = 5; g.param[i] = f; g.grad[i] = f; g.state1[i] = f; g.state2[i] = f; g.target[i] = f; }
  g.step = a; g.lr = 1e-4; g.alpha_or_beta1 = 0.9; g.beta2 = 0.999; g.eps = 1e-8; g.max_grad_norm = 0.5; g.tau = 0.5;
  MMOptGroup o;
#define OPT_REFUSED(what, change, groups, n, K, mask) \
  o = g; change; last_error[0] = 0; \
  expect(mm_opt_step_bank(groups, n, K, mask, nullptr) == MM_ERR_INVALID_ARG && last_error[0] != 0, what)
  OPT_REFUSED("opt: groups NULL", (void)0, nullptr, 1, 2, 0);
  OPT_REFUSED("opt: n_groups 0", (void)0, &o, 0, 2, 0);
  OPT_REFUSED("opt: n_groups 5", (void)0, &o, MM_OPT_MAX_GROUPS + 1, 2, 0);
  OPT_REFUSED("opt: K 0", (void)0, &o, 1, 0, 0);
  OPT_REFUSED("opt: K 65", (void)0, &o, 1, MM_BANK_MAX_GROUPS + 1, 0);
  OPT_REFUSED("opt: unknown algo", o.algo = 3, &o, 1, 2, 0);
  OPT_REFUSED("opt: n_tensors 17", o.n_tensors = MM_OPT_MAX_TENSORS + 1, &o, 1, 2, 0);
  OPT_REFUSED("opt: a negative count", o.count[1] = -1, &o, 1, 2, 0);
  OPT_REFUSED("opt: param NULL", o.param[0] = nullptr, &o, 1, 2, 0);
  OPT_REFUSED("opt: grad NULL", o.grad[1] = nullptr, &o, 1, 2, 0);
  OPT_REFUSED("opt: state1 NULL", o.state1[0] = nullptr, &o, 1, 2, 0);
  OPT_REFUSED("opt: Adam without state2", o.state2[1] = nullptr, &o, 1, 2, 0);
  OPT_REFUSED("opt: Adam without step", o.step = nullptr, &o, 1, 2, 0);
  OPT_REFUSED("opt: a member blends without a target", o.target[0] = nullptr, &o, 1, 2, 2);
  OPT_REFUSED("opt: a misaligned pointer", o.param[0] = (float *)((char *)f + 2), &o, 1, 2, 0);
  OPT_REFUSED("opt: lr < 0", o.lr = -1.0, &o, 1, 2, 0);
  OPT_REFUSED("opt: eps 0", o.eps = 0.0, &o, 1, 2, 0);
  OPT_REFUSED("opt: beta1 1", o.alpha_or_beta1 = 1.0, &o, 1, 2, 0);
  OPT_REFUSED("opt: beta2 1", o.beta2 = 1.0, &o, 1, 2, 0);
  OPT_REFUSED("opt: tau 2 with a member that blends", o.tau = 2.0, &o, 1, 2, 1);
  OPT_REFUSED("opt: max_grad_norm NaN", o.max_grad_norm = std::strtod("nan", nullptr), &o, 1, 2, 0);
  o = g; o.n_tensors = 0;
  expect(mm_opt_step_bank(&o, 1, 64, ~0ull, nullptr) == MM_OK, "opt: nothing but empty groups is a no-op");
  std::printf("%d checks, %d failed\n", checks, failures);
  return failures ? 1 : 0;
}
