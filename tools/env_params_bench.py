#!/usr/bin/env python3
"""What per-env cbf_eta / cbf_tau / HEADWAY_TIME (include/mm_env_params.h) cost and save, at BASELINE's shape.

    python tools/env_params_bench.py [--parent-lib PATH/libmm_hip.so] [--E 65536] [--N 8] [--steps 100] [--rounds 5]
                                     [--out profiles/env_params/bench.json]

merge-multi-agent-v1, MASS, E envs x N CAVs, auto-reset, bench.py's action distribution and stationary batch (episode
phases staggered by env id, one episode length rolled untimed), in both QP modes.  Times ms per step of

    a  the parent commit's library (--parent-lib; left out: "not measured"), no planes
    b  this library, no planes
    c  this library, planes equal to the config's values (the PENV kernels; same results as b)
    d  eight uniform batches of E / 8 envs stepped one after another: a K = 8 point sweep without planes

in one process: the variants are built once, warmed up, and then timed in `rounds` alternating windows of `steps` steps
each (the order within a round rotates), a window between two device events with a synchronise at its end.  Reports the median and the min / max of every
variant's windows, c / b, d / c, and whether b's median lies inside the spread of a's windows.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from marl_mass_amd import _cabi as abi  # noqa: E402
from marl_mass_amd.vec_env import BatchedMergeEnv, hip_library  # noqa: E402

SKIP = ("agents_info", "action_mask", "crashed")  # as bench.py: outputs the rollout loop does not consume


class Variant(object):
    """One or more env batches that together step E envs; step() = one policy step of all of them."""

    def __init__(self, clib, E, N, parts, qp, planes, dev):
        cfg = {"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}
        self.envs = []
        per = E // parts
        for k in range(parts):
            kw = dict(config=cfg, cbf_eta=0.03125, cbf_tau=0.5, seed=1000, auto_reset=True, qp_solver=qp, first_env=k * per,
                      skip_outputs=SKIP)
            if planes:
                kw["env_params"] = {}
            env = BatchedMergeEnv(clib, per, N, device=dev, **kw)
            env.reset()
            ge = torch.arange(k * per, (k + 1) * per, dtype=torch.int64, device=dev)
            env.env_i32[abi.EP["STEPS"]] = ((ge * 37) % env.T).to(torch.int32)
            self.envs.append(env)
        g = torch.Generator(device=dev).manual_seed(123)
        p = torch.tensor([0.1, 0.6, 0.1, 0.1, 0.1], device=dev)
        ring = [torch.multinomial(p, E * N, True, generator=g).view(E, N).int() for _ in range(16)]
        self.rings = [[a[k * per:(k + 1) * per].contiguous() for a in ring] for k in range(parts)]
        self.t = 0

    def step(self, n):
        for _ in range(n):
            for env, ring in zip(self.envs, self.rings):
                env.step(ring[self.t % 16])
            self.t += 1

    def window(self, n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        self.step(n)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / n

    def state(self):
        return torch.cat([e.f64.nan_to_num() for e in self.envs], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libmm_hip.so built from the parent commit (variant a)")
    ap.add_argument("--E", type=int, default=65536)
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--ipm-steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "env_params", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("env_params_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    new = hip_library()
    parent = abi.CLib(a.parent_lib) if a.parent_lib else None
    res = {"E": a.E, "N": a.N, "shield": "MASS", "rounds": a.rounds, "device": torch.cuda.get_device_name(dev),
           "unit": "ms per step of all E envs", "modes": {}}
    for qp, steps in (("exact", a.steps), ("ipm", a.ipm_steps)):
        names = (["a"] if parent else []) + ["b", "c", "d"]
        v = {}
        if parent:
            v["a"] = Variant(parent, a.E, a.N, 1, qp, False, dev)
        v["b"] = Variant(new, a.E, a.N, 1, qp, False, dev)
        v["c"] = Variant(new, a.E, a.N, 1, qp, True, dev)
        v["d"] = Variant(new, a.E, a.N, 8, qp, False, dev)
        for n in names:  # stationary batch + warm-up, the same number of steps for every variant
            v[n].step(v[n].envs[0].T + a.warmup)
        torch.cuda.synchronize()
        same = {n: bool(torch.equal(v[n].state(), v["b"].state())) for n in names}  # (faster and different is not faster)
        win = {n: [] for n in names}
        for r in range(a.rounds):  # (the order rotates: no variant always runs behind the same neighbour)
            for n in names[r % len(names):] + names[:r % len(names)]:
                win[n].append(v[n].window(steps))
        for n in names:
            for env in v[n].envs:
                env.poll_errors()
        med = {n: statistics.median(win[n]) for n in names}
        m = {"steps_per_window": steps, "state_equals_b_after_warmup": same,
             "variants": {n: {"median": round(med[n], 4), "min": round(min(win[n]), 4), "max": round(max(win[n]), 4),
                              "windows": [round(x, 4) for x in win[n]]} for n in names},
             "c_over_b": round(med["c"] / med["b"], 4), "d_over_c": round(med["d"] / med["c"], 4)}
        if parent:
            m["b_within_spread_of_a"] = bool(min(win["a"]) <= med["b"] <= max(win["a"]))
            m["b_over_a"] = round(med["b"] / med["a"], 4)
        else:
            m["variants"]["a"] = "not measured"
        res["modes"][qp] = m
        for n in names:
            for env in v[n].envs:
                env.close()
        del v
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
