#!/usr/bin/env python3
"""Timing of the hidden-512 actor on the device (include/mm_policy_wide.h), at E envs x 8 agents, n_s 30, n_a 5:

  (a) mm_policy_act at hidden 512 (policy_wide_kernel: forward + sample, one launch + the counter bump);
  (b) what DeviceRollout does for such an actor without the fused entry: the ActorNetwork forward + mm_sample_actions;
  (c) DeviceRollout.interact() with actor and critic at hidden 512 on the steer_vel env, eager and hipGraph-replayed.

    python tools/policy_wide_bench.py [E] [--steps T] [--json out.json]

(a) and (b): device time from events, `windows` windows of `reps` back-to-back calls after a warm-up, in the same process; the
mean and the lowest and highest window are reported, and beside them the peak of torch's allocator over one call
(max_memory_allocated above what was allocated before it).  The project's A/B bar for routing 512 actors through the kernel:
mean(a) < mean(b) by more than 5 x the larger of the two window spreads.  (c): wall clock after a synchronise, per policy step.
TFLOP/s is MFMA FLOP issued (4608 v_mfma_f32_32x32x2_f32 per 32-agent tile: 4096 of fc2, 256 of fc1, 256 of fc1 again for the
second half of fc2's outputs) against the 157 TFLOP/s f32-MFMA peak.
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from marl_mass_amd import VecMergeEnv, hip_library  # noqa: E402
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork, DeviceRollout  # noqa: E402

PEAK_TFLOPS = 157.0
MFMA_PER_TILE, FLOP_PER_MFMA = 4096 + 2 * 256, 32 * 32 * 2 * 2


def windows_ms(fn, windows=5, reps=20):
    """Per-call device time of each window, after a warm-up of one window."""
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record(); t1.synchronize()
        out.append(t0.elapsed_time(t1) / reps)
    return out


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def stats(w):
    return {"mean_ms": sum(w) / len(w), "min_ms": min(w), "max_ms": max(w), "windows_ms": w}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("E", nargs="?", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-rollout", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    E, N, S, A, T = args.E, 8, 30, 5, args.steps
    torch.manual_seed(0)
    net = ActorNetwork(S, 512, A).cuda()
    clib = hip_library()
    clib.require_policy_wide()
    n = E * N
    obs = torch.randn(n, S, device="cuda").contiguous()
    acts = torch.empty(n, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    w = [t.detach().contiguous().data_ptr() for m in (net.fc1, net.fc2, net.fc3) for t in (m.weight, m.bias)]

    def fused():
        clib.check(clib.lib.mm_policy_act(obs.data_ptr(), n, S, *w, 512, A, 7, ctr.data_ptr(), acts.data_ptr(), None, stream))

    def torch_path():
        with torch.no_grad():
            lp = net(obs).contiguous()
        clib.check(clib.lib.mm_sample_actions(lp.data_ptr(), n, A, 7, ctr.data_ptr(), acts.data_ptr(), stream))

    a, b = stats(windows_ms(fused)), stats(windows_ms(torch_path))
    a["peak_alloc_bytes"], b["peak_alloc_bytes"] = peak_bytes(fused), peak_bytes(torch_path)
    tiles = (n + 31) // 32
    flop = tiles * MFMA_PER_TILE * FLOP_PER_MFMA
    a["mfma_gflop_issued"] = flop / 1e9
    a["floor_ms_at_peak"] = flop / (PEAK_TFLOPS * 1e12) * 1e3
    a["tflops"] = flop / (a["mean_ms"] * 1e-3) / 1e12
    a["share_of_peak"] = a["tflops"] / PEAK_TFLOPS
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    res = {"E": E, "N": N, "n_s": S, "n_a": A, "agents": n, "mm_policy_act_hidden512": a, "torch_forward_plus_sample": b,
           "difference_ms": b["mean_ms"] - a["mean_ms"], "larger_window_spread_ms": spread,
           "bar_met": bool(a["mean_ms"] < b["mean_ms"] and b["mean_ms"] - a["mean_ms"] > 5 * spread)}
    if not args.no_rollout:
        kw = dict(config={"safety_guarantee": "cbf-av", "HEADWAY_TIME": 0.5, "lateral_control": "steer_vel"}, seed=9, auto_reset=True)
        critic = CriticNetwork(S, A, 512).cuda()
        for fused_policy in (True, False):
            for graph in (False, True):
                ro = DeviceRollout(VecMergeEnv(E, N, **kw), net, critic, roll_out_n_steps=T, use_graph=graph, fused_policy=fused_policy)
                assert ro.fused_policy == fused_policy
                ro.interact(); ro.interact(); torch.cuda.synchronize()
                t0 = time.perf_counter(); ro.interact(); ro.interact(); torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / 2
                res["interact_%s_%s_ms_per_step" % ("fused" if fused_policy else "module", "graph" if graph else "eager")] = dt * 1e3 / T
                del ro
                torch.cuda.empty_cache()
        res["steps"] = T
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
