#!/usr/bin/env python3
"""Timing of one agent step's gradients and optimiser step of the hidden-512 actor and critic (include/mm_policy_wide_train.h)
at n samples, n_s 30, 5 actions:

  (a) PPOLearner.loss_and_grad (both networks, per-sample form) + PPOLearner._step(): mm_policy_wide_train -- prep, then per
      network kernel A (per-sample forward / backward), kernel B (weight-gradient contractions), kernel C (fold) -- and the
      clip + RMSprop tail (torch's, or with --fused the one mm_opt_step launch);
  (b) what trains these networks without the library: float32 torch autograd of the same flat objective on copies of the same
      modules, clip_grad_norm_ and torch.optim.RMSprop.

Both run in the same process, alternating window by window, after a warm-up of every shape; a window is as many back-to-back
calls as fill 0.5 s, timed by device events; medians and the spread of the windows are reported.

    python tools/policy_wide_train_bench.py [--sizes 102400 524288] [--json out.json] [--fused]
    python tools/policy_wide_train_bench.py --sizes 524288 --kernel-stats stats.csv --json out.json
    python tools/policy_wide_train_bench.py --sharded [--chunk 65536] --json profiles/wide_sharded/bench.json

--sharded times the rank-sharded entries instead, per size on the same inputs and in passes of --chunk samples: (c) the chunked
entry (PPOLearner.loss_and_grad under the budget of that chunk), (d) shard_block + finish_shards with one block whose B is its
own count (mm_policy_wide_train_partial + mm_policy_wide_train_finish at R = 1: the same results bit for bit) and (e)
finish_shards alone over R = 8 copies of that block (B set to the eight local counts' sum), with the same windows.

Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python
tools/policy_wide_train_bench.py --sizes N --profile-run` run; pass its *_kernel_stats.csv back with --kernel-stats and the
JSON gets each kernel's mean time next to its FLOP and bytes from the shapes, and its share of the f32-MFMA peak
(157 TFLOP/s) and of the HBM bandwidth (6.3 TB/s).
"""
import argparse
import copy
import csv
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from marl_mass_amd import hip_library  # noqa: E402
from marl_mass_amd.learner import PPOLearner  # noqa: E402
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork  # noqa: E402

PEAK_TFLOPS, PEAK_GBS = 157.0, 6300.0
MFMA_FLOP = 32 * 32 * 2 * 2  # v_mfma_f32_32x32x2_f32
H, S, A = 512, 30, 5
ROW_BYTES = (32 + 4 * H + 16) * 4                                # MM_POLICY_WIDE_TRAIN_ROW_BYTES
PARTIAL_BYTES = (H * (H + 32) + 16 * H + H * 32 + H + 16 + H) * 4  # MM_POLICY_WIDE_TRAIN_PARTIAL_BYTES
MAX_SLICES, MIN_SLICE_TILES = 48, 2
WINDOW_S = 0.5


def slices_of(n):
    tiles = (n + 31) // 32
    per = max(MIN_SLICE_TILES, (tiles + MAX_SLICES - 1) // MAX_SLICES)
    return tiles, max(1, (tiles + per - 1) // per)


def kernel_model(n):
    """Static work per launch from the shapes: MFMA FLOP as issued (padding and the recomputed fc1 included), the bytes that
    have to cross HBM (observations, the scratch rows written or read, the partial blocks) and the bytes re-read from the
    caches (kernel A: fc2's 1 MiB and its transpose once per tile; kernel B: every row operand is read by several output
    blocks).  Keys are substrings of the kernel names as rocprofv3 prints them."""
    tiles, slices = slices_of(n)
    fwd = 4 * 16 * 16 + 16 * 16 * 16  # per tile: fc1 once per quarter (4 x 256 MFMAs), fc2 (4096)
    bwd = 16 * 16 * 16                # the W2^T contraction
    out = {}
    for tag in ("<false, true, true>", "<true, true, true>"):
        out["policy_wide_sample_kernel" + tag] = {
            "flop": tiles * (fwd + bwd) * MFMA_FLOP,
            # x, h1, h2, dz2, dz1, dhead written; h2, dz2 (16 x per quarter walk: from the caches), h1 read back
            "hbm_bytes": n * (S * 4 + ROW_BYTES + 3 * H * 4), "cache_bytes": tiles * 2 * H * H * 4 + n * 3 * H * 4}
    for tag in ("<false, false, true>", "<true, false, true>", "<false, false, false>", "<true, false, false>"):
        out["policy_wide_sample_kernel" + tag] = {"flop": tiles * fwd * MFMA_FLOP, "hbm_bytes": n * (S * 4 + 8),
                                                  "cache_bytes": tiles * H * H * 4}
    for crit, tag in ((0, "<false>"), (1, "<true>")):
        per_pair = 16 * 16 + 16 * (2 + crit)  # per 2 samples: dW2's 16 x 16 tiles; per row tile dW1, the head tile (+ the one-hot tile)
        # each slice's rows are read by 10 output blocks: dz2 by all, h1 by 2 (its four column groups once per row half)
        out["policy_wide_wgrad_kernel" + tag] = {"flop": tiles * 16 * per_pair * MFMA_FLOP,
                                                 "hbm_bytes": n * ROW_BYTES + slices * PARTIAL_BYTES,
                                                 "cache_bytes": n * (9 * H + 1 * H) * 4}
    out["policy_wide_fold_kernel"] = {"flop": 0, "hbm_bytes": slices * PARTIAL_BYTES, "cache_bytes": 0}
    out["policy_wide_prep_kernel"] = {"flop": 0, "hbm_bytes": 2 * 3 * H * H * 4, "cache_bytes": 0}
    return out


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record(); t1.synchronize()
    return t0.elapsed_time(t1) / reps


def alternate(fns, windows):
    """fns: {name: callable}.  Warm-up, then `windows` rounds in which every callable gets one window of >= WINDOW_S of
    back-to-back calls; {name: {"median_ms", "min_ms", "max_ms", "reps", "windows"}}."""
    reps = {}
    for name, fn in fns.items():
        fn(); fn(); torch.cuda.synchronize()
        reps[name] = max(2, int(math.ceil(WINDOW_S * 1e3 / timed(fn, 3))))
    got = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            got[name].append(timed(fn, reps[name]))
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "reps": reps[name], "windows": windows}
            for name, v in got.items()}


def paths(n, fused):
    torch.manual_seed(0)
    actor, critic = ActorNetwork(S, H, A).cuda(), CriticNetwork(S, A, H, 1).cuda()
    learner = PPOLearner(actor, critic, hip_library(), fused_step=fused)
    with torch.no_grad():  # networks that have moved away from their targets: ratios off 1
        for p in list(actor.parameters()) + list(critic.parameters()):
            p.add_(0.01 * torch.randn_like(p))
    obs = torch.randn(n, S, device="cuda")
    act = torch.randint(0, A, (n,), device="cuda", dtype=torch.int32)
    ret = torch.randn(n, device="cuda")
    old = learner.old_log_probs(obs, act)
    adv = learner.advantages(obs, act, ret)

    def kernel_path():
        learner.loss_and_grad(obs, act, ret, old, advantages=adv)
        learner._step()

    def grad_only():
        learner.loss_and_grad(obs, act, ret, old, advantages=adv)

    twin_a, twin_c = copy.deepcopy(actor), copy.deepcopy(critic)
    opt_a, opt_c = torch.optim.RMSprop(twin_a.parameters(), lr=1e-4), torch.optim.RMSprop(twin_c.parameters(), lr=1e-4)
    idx = act.long().unsqueeze(1)
    oh = torch.nn.functional.one_hot(act.long(), A).float()

    def torch_path():
        opt_a.zero_grad(set_to_none=True); opt_c.zero_grad(set_to_none=True)
        logp = twin_a(obs).gather(1, idx).squeeze(1)
        ratio = torch.exp(logp - old)
        (-torch.mean(torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv))).backward()
        torch.nn.utils.clip_grad_norm_(twin_a.parameters(), 0.5)
        opt_a.step()
        torch.nn.functional.mse_loss(twin_c(obs, oh), ret.unsqueeze(1)).backward()
        torch.nn.utils.clip_grad_norm_(twin_c.parameters(), 0.5)
        opt_c.step()

    return {"library_loss_and_grad_plus_step": kernel_path, "torch_autograd_clip_rmsprop": torch_path,
            "library_loss_and_grad": grad_only}


def sharded_paths(n, chunk):
    """The three timings of --sharded on one batch of n samples in passes of `chunk` (the budget of exactly that chunk)."""
    torch.manual_seed(0)
    clib = hip_library()
    actor, critic = ActorNetwork(S, H, A).cuda(), CriticNetwork(S, A, H, 1).cuda()
    budget = clib.policy_wide_train_chunked_scratch_bytes(n, chunk)
    learner = PPOLearner(actor, critic, clib, scratch_budget_bytes=budget)
    with torch.no_grad():
        for p in list(actor.parameters()) + list(critic.parameters()):
            p.add_(0.01 * torch.randn_like(p))
    obs = torch.randn(n, S, device="cuda")
    act = torch.randint(0, A, (n,), device="cuda", dtype=torch.int32)
    ret = torch.randn(n, device="cuda")
    old = learner.old_log_probs(obs, act)
    adv = learner.advantages(obs, act, ret)
    count = torch.tensor([n], dtype=torch.int32, device="cuda")
    block = torch.empty(1, learner.shard_doubles(), dtype=torch.float64, device="cuda")

    def chunked():
        learner.loss_and_grad(obs, act, ret, old, advantages=adv)

    def partial_finish():
        learner.shard_block(obs, act, ret, old, count, advantages=adv, out=block[0])
        learner.finish_shards(block)

    chunked()
    want = [p.grad.clone() for p in list(actor.parameters()) + list(critic.parameters())]
    partial_finish()
    torch.cuda.synchronize()
    assert chunk >= n or learner._chunks[n][0] == chunk, learner._chunks
    same = all(torch.equal(p.grad, w) for p, w in zip(list(actor.parameters()) + list(critic.parameters()), want))
    eight = block.repeat(8, 1)
    eight[:, 0] = 8 * n  # B: the eight local counts add up to it

    def finish_8():
        learner.finish_shards(eight)

    loss = learner.finish_shards(eight)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()), "the eight blocks must pass the header check"
    fns = {"chunked": chunked, "partial_plus_finish_r1": partial_finish, "finish_r8": finish_8}
    return fns, {"chunk": learner._chunks[n][0], "passes": (n + chunk - 1) // chunk, "r1_bits_equal_chunked": same,
                 "scratch_MB": budget / 2 ** 20, "block_MB": block.numel() * 8 / 1e6}


def sharded_main(args):
    res = {"n_s": S, "n_a": A, "hidden": H, "window_s": WINDOW_S, "chunk": args.chunk, "sizes": {}}
    for n in args.sizes:
        fns, info = sharded_paths(n, args.chunk)
        r = alternate(fns, args.windows)
        r.update(info)
        spread = lambda v: (v["max_ms"] - v["min_ms"]) / v["median_ms"]  # noqa: E731
        r["spread"] = {k: spread(r[k]) for k in fns}
        r["r1_over_chunked"] = r["partial_plus_finish_r1"]["median_ms"] / r["chunked"]["median_ms"]
        r["finish_r8_over_chunked"] = r["finish_r8"]["median_ms"] / r["chunked"]["median_ms"]
        res["sizes"][str(n)] = r
        del fns
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sharded", action="store_true", help="time the chunked entry, partial + finish at R = 1 and finish at R = 8")
    ap.add_argument("--chunk", type=int, default=65536, help="--sharded: samples per pass")
    ap.add_argument("--sizes", nargs="+", type=int, default=[102400, 524288])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--fused", action="store_true", help="the tail as one mm_opt_step launch (fused_step=True)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-run", action="store_true", help="a few calls of each path only: the run to put under rocprofv3")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3's *_kernel_stats.csv of a --profile-run at ONE size")
    args = ap.parse_args()
    if args.sharded:
        return sharded_main(args)
    res = {"n_s": S, "n_a": A, "hidden": H, "fused_step": args.fused, "window_s": WINDOW_S, "sizes": {}}
    for n in args.sizes:
        fns = paths(n, args.fused)
        if args.profile_run:
            for fn in fns.values():
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            continue
        r = alternate(fns, args.windows)
        r["scratch_MB"] = hip_library().policy_wide_train_scratch_bytes(n) / 2 ** 20
        r["torch_over_library"] = r["torch_autograd_clip_rmsprop"]["median_ms"] / r["library_loss_and_grad_plus_step"]["median_ms"]
        res["sizes"][str(n)] = r
        del fns
        torch.cuda.empty_cache()
    if args.kernel_stats:
        n = args.sizes[0]
        model = kernel_model(n)
        res["kernels_n"] = n
        res["kernels"] = {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                for k, m in model.items():
                    if k in row["Name"]:
                        ms = float(row["AverageNs"]) / 1e6
                        flops, hbm = m["flop"] / ms / 1e9 / PEAK_TFLOPS, m["hbm_bytes"] / ms / 1e6 / PEAK_GBS
                        res["kernels"][k] = {"calls": int(row["Calls"]), "mean_ms": ms, "gflop": m["flop"] / 1e9,
                                             "hbm_MB": m["hbm_bytes"] / 1e6, "cache_MB": m["cache_bytes"] / 1e6,
                                             "frac_mfma_peak": flops, "frac_hbm_peak": hbm,
                                             "bound_by": "mfma" if m["flop"] / PEAK_TFLOPS / 1e3 > m["hbm_bytes"] / PEAK_GBS else "hbm"}
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
