#!/usr/bin/env python3
"""Cost of the "dmc" safety supervisor on merge-multi-agent-v0: the lane-parallel default form against its literal
one-lane-per-env form and against the "priority" supervisor, on the same states.

    python tools/dmc_bench.py [--E 4096 16384 65536] [--N 8] [--steps 20] [--warmup 3] [--advance 15] [--out FILE]

For every batch size and traffic mix (N CAVs, and N/2 CAVs + N/2 HDVs): a batch is reset, advanced `advance` supervised steps
with FASTER-biased actions (so that lookaheads crash), and then, WITHOUT stepping further, the supervise launch alone is timed
in the three variants with device events around a synchronised window of `steps` launches after `warmup` (device Philox
draws).  The window is repeated `--repeats` times; median and spread are reported.  ms per supervised env-step comes from a
separate window of env.step() calls (auto_reset on).  Also reported: the share of envs with at least one replacement and
the number of (vehicle, candidate) pairs scored, since the cost depends on them.  One JSON line per configuration; --out
collects them in a file.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from marl_mass_amd import VecMergeEnv  # noqa: E402
from marl_mass_amd import _cabi as abi  # noqa: E402


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


def timed(fn, args):
    xs = [window(fn, args.steps, args.warmup if k == 0 else 1) for k in range(args.repeats)]
    return {"ms": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def make(E, N, n_hdv, sg):
    return VecMergeEnv(E, N, env_id="merge-multi-agent-v0", config={"safety_guarantee": sg, "HEADWAY_TIME": 0.5}, auto_reset=True,
                       seed=1, n_hdv=n_hdv, enable_dmc=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, nargs="+", default=[4096, 16384, 65536])
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--advance", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    p = torch.tensor([0.05, 0.1, 0.05, 0.75, 0.05], device="cuda:0")
    rows = []
    for E in args.E:
        for n_hdv in (0, args.N // 2):
            N = args.N
            acts = [torch.multinomial(p, E * N, True, generator=g).view(E, N).int() for _ in range(args.advance + 1)]
            dmc, prio = make(E, N, n_hdv, "dmc"), make(E, N, n_hdv, "priority")
            dmc.reset()
            for a in acts[:-1]:
                dmc.step(a)
            prio.state.copy_(dmc.state)  # the same states for the yardstick
            a = acts[-1]
            res = {"E": E, "N": N, "n_cav": N - n_hdv, "n_hdv": n_hdv, "advance": args.advance}
            new = dmc.supervise(a, trace=True)[0]
            ctrl = dmc.u8[abi.B["KIND"]] == 1
            res["share_envs_replaced"] = round(float(((new != a) & ctrl).any(1).float().mean()), 4)
            crashed = dmc.dmc_trace[:, :, 2] >= 0
            res["vehicles_crashing"] = int(crashed.sum())
            res["pairs_scored"] = int((~torch.isnan(dmc.dmc_trace[:, :, 8:13])).sum())
            res["supervise_dmc_default"] = timed(lambda: dmc.supervise(a), args)
            res["supervise_dmc_literal"] = timed(lambda: dmc.supervise(a, literal=True), args)
            res["supervise_priority"] = timed(lambda: prio.supervise(a), args)
            res["default_over_literal"] = round(res["supervise_dmc_literal"]["ms"] / res["supervise_dmc_default"]["ms"], 3)
            res["step_dmc"] = timed(lambda: dmc.step(a), args)
            res["step_priority"] = timed(lambda: prio.step(a), args)
            dmc.poll_errors()
            prio.poll_errors()
            rows.append(res)
            print(json.dumps(res), flush=True)
            del dmc, prio
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/dmc_bench.py", "device": torch.cuda.get_device_name(0), "args": vars(args), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
