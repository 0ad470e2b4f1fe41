#!/usr/bin/env python3
"""Throughput of merge-multi-agent-hdv-v1 (the all-HDV IDM baseline) on the device.

    python tools/idm_bench.py [--E 65536] [--N 12] [--density 3] [--steps 50] [--warmup 5]

E envs x N slots with the device count draw of traffic_density `density` and auto-reset, stepped with step(None).  Reports
ms per batched step, env-steps/s and vehicle-steps/s (occupied slots only) from device events around `steps` steps, as
one JSON line.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from marl_mass_amd import VecMergeEnv, _cabi as abi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, default=65536)
    ap.add_argument("--N", type=int, default=12)
    ap.add_argument("--density", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    env = VecMergeEnv(a.E, a.N, env_id="merge-multi-agent-hdv-v1", config={"traffic_density": a.density},
                      draw_counts=True, auto_reset=True, seed=1)
    env.reset()
    for _ in range(a.warmup):
        env.step(None)
    torch.cuda.synchronize()
    occupied = 0
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kind = env.u8[abi.B["KIND"]]
    t0.record()
    for _ in range(a.steps):
        env.step(None)
    t1.record()
    t1.synchronize()
    occupied = int((kind != 0).sum())  # (vehicles per env change with every re-spawn; the end-of-window count is representative)
    ms = t0.elapsed_time(t1) / a.steps
    env.poll_errors()
    print(json.dumps({"env": "merge-multi-agent-hdv-v1", "E": a.E, "N": a.N, "density": a.density, "steps": a.steps,
                      "ms_per_step": round(ms, 4), "env_steps_per_s": round(a.E / ms * 1e3, 1),
                      "vehicle_steps_per_s": round(occupied / ms * 1e3, 1), "vehicles": occupied}))


if __name__ == "__main__":
    main()
