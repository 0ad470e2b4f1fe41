#!/usr/bin/env python3
"""Timing of the learners' fused optimiser step (include/mm_opt_step.h) against the torch tail it replaces:

  (a) the bare mm_opt_step launch: one group (the shared actor-critic's twelve tensors) and two groups (MAPPO's actor and
      critic), RMSprop and Adam, with and without the soft update in the same launch;
  (b) one agent step of train(form="reference") of SharedPPOLearner and PPOLearner with fused_step off -- clip_grad_norm_,
      torch.optim and the per-tensor blend: the yardstick -- and on, at n samples per agent, without and with the soft update.

    python tools/opt_step_bench.py [--n 100 4096 65536 524288] [--json out.json] [--launch-trace kernel_trace.csv]
    python tools/opt_step_bench.py --launches          # the run to put under rocprofv3 (see below)

Device time by events over windows of back-to-back calls after a warm-up, as in tools/policy_train_bench.py: mean (lowest
window, highest window).  At small n the step is bound by launches and by the host, which the event window includes.

Launch counts per agent step come from ONE `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python
tools/opt_step_bench.py --launches` run: that mode runs a few agent steps of every (learner, path) with the library's
diagnostic math_kernel between the segments as a marker; pass its *_kernel_trace.csv back with --launch-trace and the JSON
gets the number of kernel launches per agent step of each segment.
"""
import argparse
import csv
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from marl_mass_amd import hip_library  # noqa: E402
from marl_mass_amd.learner import PPOLearner, SharedPPOLearner  # noqa: E402
from marl_mass_amd.rollout import ActorCriticNetwork, ActorNetwork, CriticNetwork  # noqa: E402

S, A = 30, 5
SEGMENTS = [(kind, fused, soft) for kind in ("shared", "ppo") for fused in (False, True) for soft in (False, True)]
TRACE_STEPS = 8


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
    return {"mean_ms": sum(out) / windows, "min_ms": min(out), "max_ms": max(out)}


def make_learner(kind, fused, optimizer_type="rmsprop"):
    torch.manual_seed(0)
    kw = dict(fused_step=fused, optimizer_type=optimizer_type, target_tau=0.5, target_update_steps=1)
    if kind == "shared":
        net = ActorCriticNetwork(S, A, 128, 1, state_split=True).cuda()
        learner, nets = SharedPPOLearner(net, hip_library(), **kw), [net]
    else:
        actor, critic = ActorNetwork(S, 128, A).cuda(), CriticNetwork(S, A, 128, 1).cuda()
        learner, nets = PPOLearner(actor, critic, hip_library(), **kw), [actor, critic]
    with torch.no_grad():  # networks that have moved away from their targets: ratios off 1
        for net in nets:
            for p in net.parameters():
                p.add_(0.01 * torch.randn_like(p))
    return learner


def batch(n):
    g = torch.Generator().manual_seed(1)
    return (torch.randn(n, 1, S, generator=g).cuda(), torch.randint(0, A, (n, 1), generator=g, dtype=torch.int32).cuda(),
            torch.randn(n, 1, generator=g).cuda())


def agent_step(learner, data, soft):
    """One agent step: train() on one agent column; n_episodes 1 triggers the soft update (target_update_steps is 1)."""
    return lambda: learner.train(*data, n_episodes=1 if soft else 0)


def bare(n_groups, algo, soft):
    """The bare launch on the learners' own tensor sizes, gradients given."""
    learner = make_learner("shared" if n_groups == 1 else "ppo", True, algo)
    for f in learner._fused:
        for p in f.params:
            p.grad.normal_()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lambda: learner.clib.opt_step([f.fill(0.5, 0.5, soft) for f in learner._fused], stream)


def marker(lib, buf):
    lib.check(lib.lib.mm_math_eval(0, 1, buf.data_ptr(), None, buf.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


def run_launches(n):
    """The rocprofv3 run: marker, TRACE_STEPS agent steps of a segment, marker, ... in the order of SEGMENTS (every learner
    warmed up before the first marker)."""
    lib, data = hip_library(), batch(n)
    buf = torch.zeros(1, dtype=torch.float64, device="cuda")
    steps = []
    for kind, fused, soft in SEGMENTS:
        step = agent_step(make_learner(kind, fused), data, soft)
        step(); step()
        steps.append(step)
    torch.cuda.synchronize()
    for step in steps:
        marker(lib, buf)
        for _ in range(TRACE_STEPS):
            step()
    marker(lib, buf)
    torch.cuda.synchronize()


def launches_per_step(trace_csv):
    """Kernel launches per agent step of every segment of a --launches run, from rocprofv3's kernel trace."""
    with open(trace_csv) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if "math_kernel" in r["Kernel_Name"]]
    if len(marks) != len(SEGMENTS) + 1:
        raise ValueError("expected %d markers in %s, found %d" % (len(SEGMENTS) + 1, trace_csv, len(marks)))
    out = {}
    for (kind, fused, soft), lo, hi in zip(SEGMENTS, marks[:-1], marks[1:]):
        names = [r["Kernel_Name"] for r in rows[lo + 1:hi]]
        out["%s_%s%s" % (kind, "fused" if fused else "torch", "_soft" if soft else "")] = {
            "launches_per_agent_step": (hi - lo - 1) / TRACE_STEPS,
            "opt_step_kernel_per_agent_step": sum("opt_step_kernel" in k for k in names) / TRACE_STEPS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", nargs="*", type=int, default=[100, 4096, 65536, 524288])
    ap.add_argument("--json", default=None)
    ap.add_argument("--launches", action="store_true", help="only the marked agent steps, for a rocprofv3 --kernel-trace run")
    ap.add_argument("--launch-trace", default=None, help="the *_kernel_trace.csv of a --launches run")
    args = ap.parse_args()
    if args.launches:
        return run_launches(100)
    res = {"n_s": S, "n_a": A, "bare": {}, "agent_step": {}}
    for n_groups in (1, 2):
        for algo in ("rmsprop", "adam"):
            for soft in (False, True):
                res["bare"]["%d_group%s_%s%s" % (n_groups, "s" if n_groups > 1 else "", algo, "_blend" if soft else "")] = device_ms(
                    bare(n_groups, algo, soft), reps=50)
    for n in args.n:
        data = batch(n)
        for kind in ("shared", "ppo"):
            for soft in (False, True):
                row = {}
                for fused in (False, True):
                    row["fused" if fused else "torch"] = device_ms(agent_step(make_learner(kind, fused), data, soft),
                                                                   reps=20 if n <= 65536 else 10)
                row["torch_over_fused"] = row["torch"]["mean_ms"] / row["fused"]["mean_ms"]
                # the fused windows lie wholly below the unfused ones | the fused mean is not above the unfused highest window
                row["fused_windows_below_torch_windows"] = row["fused"]["max_ms"] < row["torch"]["min_ms"]
                row["fused_mean_not_above_torch_max"] = row["fused"]["mean_ms"] <= row["torch"]["max_ms"]
                res["agent_step"]["%s_n%d%s" % (kind, n, "_soft" if soft else "")] = row
                print("%-7s n %7d soft %d  torch %.4f (%.4f - %.4f)  fused %.4f (%.4f - %.4f) ms  x%.2f" % (
                    kind, n, soft, row["torch"]["mean_ms"], row["torch"]["min_ms"], row["torch"]["max_ms"], row["fused"]["mean_ms"],
                    row["fused"]["min_ms"], row["fused"]["max_ms"], row["torch_over_fused"]), flush=True)
        del data
        torch.cuda.empty_cache()
    if args.launch_trace:
        res["launches"] = launches_per_step(args.launch_trace)
        res["launches"]["trace_steps_per_segment"] = TRACE_STEPS
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
