#!/usr/bin/env python3
"""Cost of the "priority" safety supervisor on merge-multi-agent-v0: supervised vs unsupervised steps.

    python tools/supervisor_bench.py [--E 4096 16384 65536] [--N 8] [--steps 20] [--warmup 3]

For every batch size: ms per env-step (one step of the whole batch) and agent-steps/s from device events around a
synchronised window of `steps` steps, with safety_guarantee "none" and "priority" (device Philox draws), plus the
supervisor launch alone (VecMergeEnv.supervise on the same state).  One JSON line per configuration.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from marl_mass_amd import VecMergeEnv  # noqa: E402


def window(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, nargs="+", default=[4096, 16384, 65536])
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    p = torch.tensor([0.15, 0.15, 0.1, 0.5, 0.1], device="cuda:0")
    for E in args.E:
        acts = torch.multinomial(p, E * args.N, True, generator=g).view(E, args.N).int()
        res = {"E": E, "N": args.N}
        for sg in ("none", "priority"):
            env = VecMergeEnv(E, args.N, env_id="merge-multi-agent-v0", config={"safety_guarantee": sg},
                              auto_reset=True, seed=1)
            env.reset()
            ms = window(lambda: env.step(acts), args.steps, args.warmup)
            res["ms_per_step_" + sg] = round(ms, 4)
            res["agent_steps_per_s_" + sg] = round(E * args.N / (ms * 1e-3), 1)
            if sg == "priority":
                res["ms_supervise_only"] = round(window(lambda: env.supervise(acts), args.steps, args.warmup), 4)
                replaced = int((env.supervise(acts)[0] != acts).sum())
                res["replaced_per_step"] = replaced
            env.poll_errors()
            del env
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
