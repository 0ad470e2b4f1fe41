#!/usr/bin/env python3
"""Timing of MAPPO's separate actor / critic loss + gradients on the device (include/mm_policy_train.h) at n samples, n_s 30:

  (a) PPOLearner.loss_and_grad -- mm_policy_train: prep, then per network kernel A (per-sample forward / backward) + kernel B
      (weight-gradient contractions) + kernel C (fold), device time by events;
  (b) the torch path it replaces, in the same process, float32, the O(B) form of the reference's objective: target actor
      forward, target critic forward, actor forward + backward, critic forward + backward on rollout.ActorNetwork /
      rollout.CriticNetwork;
  (c) one whole agent step of train(form="reference") (mm_policy_eval of both targets, advantage sums, both gradients, two
      clip_grad_norm_ and two RMSprop steps).

    python tools/policy_train_bench.py [n] [--json out.json] [--kernel-stats stats.csv [--stats-out trimmed.csv]]

Per-kernel times come from one `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python
tools/policy_train_bench.py` run of this same command; pass its *_kernel_stats.csv back with --kernel-stats and the JSON gets
each kernel's mean time with achieved TFLOP/s (against the 157 TFLOP/s fp32-MFMA peak) and GB/s (against 6.3 TB/s), from the
static MFMA / byte counts below.
"""
import argparse
import csv
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from marl_mass_amd import hip_library  # noqa: E402
from marl_mass_amd.learner import PPOLearner  # noqa: E402
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork  # noqa: E402

PEAK_TFLOPS, PEAK_GBS = 157.0, 6300.0
MFMA_FLOP = 32 * 32 * 2 * 2  # v_mfma_f32_32x32x2_f32
ROW_BYTES = (128 + 128 + 128 + 128 + 16 + 32) * 4  # scratch per sample: h1, dz1, h2, dz2, dhead, x
PARTIAL = 26896  # floats per partial block (kPartial)


def device_ms(fn, reps=20, windows=5):
    """Device time per call by events: `windows` windows of `reps` back-to-back calls after a warm-up; (mean, lowest window,
    highest window)."""
    fn(); fn(); torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record(); t1.synchronize()
        out.append(t0.elapsed_time(t1) / reps)
    return sum(out) / windows, min(out), max(out)


def kernel_model(n, slices=512):
    """Static work per launch: MFMA FLOP (as issued, padding included), bytes that have to cross HBM (the scratch rows, the
    observations, the partial blocks) and, apart from them, bytes re-read from the caches (kernel A: the 64 KB of W2^T
    fragments per tile, L2; kernel B: h1 is read by 4 waves of a workgroup, 3 of them from L1 / L2).  Keys are substrings of
    the kernel names as rocprofv3 prints them; slices: kMaxSlices of the build."""
    tiles = (n + 31) // 32
    a_train = 64 + 256 + 256  # fc1, fc2, the W2^T contraction, per 32 samples
    a_eval = 64 + 256
    slices = min(slices, max(1, (tiles + 1) // 2))
    out = {}
    for crit, tag in ((0, "<false, true, mm::pt::Flat"), (1, "<true, true, mm::pt::Flat")):
        out["mlp_sample_kernel" + tag] = {"flop": tiles * a_train * MFMA_FLOP, "hbm_bytes": n * (30 * 4 + ROW_BYTES),
                                          "cache_bytes": tiles * 64 * 1024}
    for crit, tag in ((0, "<false>"), (1, "<true>")):
        b_mfma = (16 + 4 * crit) + 4 + 4  # per 2 samples: dW2 (+ the one-hot tile), the head tile, dz1^T x
        out["policy_train_wgrad_kernel" + tag] = {"flop": (tiles * 16) * b_mfma * MFMA_FLOP,
                                                  "hbm_bytes": n * ROW_BYTES + slices * PARTIAL * 4, "cache_bytes": n * 3 * 128 * 4}
    for tag in ("<false, false, mm::pt::Flat", "<true, false, mm::pt::Flat"):
        out["mlp_sample_kernel" + tag] = {"flop": tiles * a_eval * MFMA_FLOP, "hbm_bytes": n * (30 * 4 + 8), "cache_bytes": 0}
    out["policy_train_fold_kernel"] = {"flop": 0, "hbm_bytes": slices * PARTIAL * 4, "cache_bytes": 0}
    out["policy_train_prep_kernel"] = {"flop": 0, "hbm_bytes": 4 * 64 * 1024, "cache_bytes": 0}
    return out


def trim_stats(src, dst, width=100):
    """Copy a rocprofv3 kernel-stats CSV with every kernel name cut to `width` characters (torch's template names run to
    several KB each) and without the rows below 0.1 % of the time, which is the form that is committed under profiles/."""
    with open(src) as f, open(dst, "w", newline="") as g:
        rows = list(csv.reader(f))
        keep = [r for r in rows[1:] if r and (float(r[4]) >= 0.1 or "policy_train" in r[0] or "mm::pt::" in r[0])]  # >= 0.1 % of the time, or ours
        csv.writer(g, quoting=csv.QUOTE_MINIMAL).writerows([[r[0][:width]] + r[1:] for r in rows[:1] + keep])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=524288)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--slices", type=int, default=512, help="kMaxSlices of the library build (mm_policy_train.hip)")
    ap.add_argument("--stats-out", default=None, help="write the trimmed copy of --kernel-stats here")
    args = ap.parse_args()
    n, S, A = args.n, 30, 5
    torch.manual_seed(0)
    actor, critic = ActorNetwork(S, 128, A).cuda(), CriticNetwork(S, A, 128, 1).cuda()
    learner = PPOLearner(actor, critic, hip_library())
    with torch.no_grad():  # networks that have moved away from their targets: ratios off 1
        for p in list(actor.parameters()) + list(critic.parameters()):
            p.add_(0.01 * torch.randn_like(p))
    obs = torch.randn(n, S, device="cuda").contiguous()
    act = torch.randint(0, A, (n,), device="cuda", dtype=torch.int32)
    ret = torch.randn(n, device="cuda")
    old = learner.old_log_probs(obs, act)
    sums = learner.advantage_sums(obs, act, ret)

    def kernel_path():
        learner.loss_and_grad(obs, act, ret, old, adv_sums=sums)

    def eval_path():
        learner.evaluate(obs, act, actor=learner.actor_target, critic=learner.critic_target)

    twin_a, twin_c = ActorNetwork(S, 128, A).cuda(), CriticNetwork(S, A, 128, 1).cuda()
    twin_a.load_state_dict(actor.state_dict()); twin_c.load_state_dict(critic.state_dict())
    idx = act.long().unsqueeze(1)
    oh = torch.nn.functional.one_hot(act.long(), A).float()

    def torch_path():
        for p in list(twin_a.parameters()) + list(twin_c.parameters()):
            p.grad = None
        with torch.no_grad():
            old_t = learner.actor_target(obs).gather(1, idx).squeeze(1)
            adv = ret.unsqueeze(1) - learner.critic_target(obs, oh)
        logp = twin_a(obs).gather(1, idx).squeeze(1)
        ratio = torch.exp(logp - old_t)
        c = torch.clamp(ratio, 0.8, 1.2)
        sp, sn = adv.clamp(min=0).sum(), adv.clamp(max=0).sum()
        (-(sp * torch.min(ratio, c) + sn * torch.max(ratio, c)).sum() / float(n) ** 2).backward()
        torch.nn.functional.mse_loss(twin_c(obs, oh), ret.unsqueeze(1)).backward()

    def agent_step():
        learner.train(obs.view(n, 1, S), act.view(n, 1), ret.view(n, 1), n_episodes=0)

    res = {"n": n, "n_s": S, "scratch_MB": hip_library().policy_train_scratch_bytes(n) / 2 ** 20}
    for name, fn, reps in (("loss_and_grad_ms", kernel_path, 20), ("eval_both_targets_ms", eval_path, 20),
                           ("torch_2_forwards_plus_2_forward_backward_ms", torch_path, 20),
                           ("train_reference_agent_step_ms", agent_step, 10)):
        res[name], res[name + "_min"], res[name + "_max"] = device_ms(fn, reps)
    # (a) takes old_logp / (S+, S-) as inputs; (b) contains the two target forwards that produce them, which on the device are
    # eval_both_targets_ms.  Like for like is (b) against (a) + the evaluation, or against the agent step (c), which also holds
    # both clip_grad_norm_ and RMSprop steps.
    res["torch_over_loss_and_grad"] = res["torch_2_forwards_plus_2_forward_backward_ms"] / res["loss_and_grad_ms"]
    res["torch_over_loss_and_grad_plus_eval"] = res["torch_2_forwards_plus_2_forward_backward_ms"] / (
        res["loss_and_grad_ms"] + res["eval_both_targets_ms"])
    res["torch_over_agent_step"] = res["torch_2_forwards_plus_2_forward_backward_ms"] / res["train_reference_agent_step_ms"]
    if args.kernel_stats:
        if args.stats_out:
            trim_stats(args.kernel_stats, args.stats_out)
        model = kernel_model(n, args.slices)
        res["kernels"] = {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                for k, m in model.items():
                    if k in row["Name"]:
                        ms = float(row["AverageNs"]) / 1e6
                        res["kernels"][k] = {"calls": int(row["Calls"]), "mean_ms": ms, "min_ms": float(row["MinNs"]) / 1e6,
                                             "max_ms": float(row["MaxNs"]) / 1e6, "tflops": m["flop"] / ms / 1e9,
                                             "frac_mfma_peak": m["flop"] / ms / 1e9 / PEAK_TFLOPS,
                                             "hbm_gbs": m["hbm_bytes"] / ms / 1e6, "frac_hbm_peak": m["hbm_bytes"] / ms / 1e6 / PEAK_GBS,
                                             "cache_gbs": m["cache_bytes"] / ms / 1e6}
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
