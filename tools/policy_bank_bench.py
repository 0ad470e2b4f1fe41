#!/usr/bin/env python3
"""Timing of the policy bank's act launch on the device (include/mm_policy_bank.h), n_s 30, n_a 5, K equal groups:

  (a) ONE mm_policy_bank_act launch over the whole batch (+ its counter bump);
  (b) what it replaces: K sequential mm_policy_act calls on the groups' slices (K launches + K counter bumps).

    python tools/policy_bank_bench.py [--json profiles/policy_bank/bench.json]

Shapes: 524 288 agents with K in {1, 4, 16, 64} and 32 768 agents with K = 16 (the population case, in which launches dominate).
Device time from events; every shape is warmed up (one window of both variants), then `windows` windows of `reps` back-to-back
calls per variant, the two variants ALTERNATING window by window in the same process.  Beside every mean stand the lowest and the
highest window and their difference (the spread); `faster_by_more_than_spread` compares the difference of the means with the
larger of the two spreads.  Staging: a workgroup stages its member's 84 KB of fragments once, so a launch stages
grid x 84 KB (grid >= K, one workgroup per CU per wave of workgroups); `staging_launch` times the bank launch with the same grid
and the same split on 256 agents per workgroup -- launch, lookup, staging and ONE tile per wave, so an upper bound of what is not
tile work -- and `staging_share` is that over the full launch's time (at 32 768 agents the full launch IS one tile per wave).
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from marl_mass_amd import _cabi as abi, hip_library  # noqa: E402
from marl_mass_amd.rollout import ActorNetwork, PolicyBank  # noqa: E402

S, A = 30, 5
SHAPES = ((524288, 1), (524288, 4), (524288, 16), (524288, 64), (32768, 16))


def window_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record(); t1.synchronize()
    return t0.elapsed_time(t1) / reps


def alternate(fns, windows, reps):
    """{name: per-call ms of each window}: a warm-up window of every variant, then the variants alternate window by window."""
    for fn in fns.values():
        window_ms(fn, reps)
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window_ms(fn, reps))
    return out


def stats(w):
    return {"mean_ms": sum(w) / len(w), "min_ms": min(w), "max_ms": max(w), "spread_ms": max(w) - min(w), "windows_ms": w}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    clib = hip_library()
    clib.require_policy_bank()
    torch.manual_seed(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    rows = []
    for n, K in SHAPES:
        members = [ActorNetwork(S, 128, A).cuda() for _ in range(K)]
        bank = PolicyBank(members)
        obs = torch.randn(n, S, device="cuda").contiguous()
        acts = torch.empty(n, dtype=torch.int32, device="cuda")
        per = n // K
        start = (ctypes.c_int64 * (K + 1))(*[k * per for k in range(K)] + [n])
        grid = (ctypes.c_int32 * (K + 1))()
        clib.check(clib.lib.mm_policy_bank_grid(K, start, grid))
        wg = [grid[k + 1] - grid[k] for k in range(K)]
        tiny = (ctypes.c_int64 * (K + 1))(*[32 * 8 * sum(wg[:k]) for k in range(K + 1)])  # 8 tiles per workgroup: the same grid
        tiny_grid = (ctypes.c_int32 * (K + 1))()
        clib.check(clib.lib.mm_policy_bank_grid(K, tiny, tiny_grid))
        assert list(tiny_grid) == list(grid) and tiny[K] <= n
        w = [[p.detach().data_ptr() for m in (a.fc1, a.fc2, a.fc3) for p in (m.weight, m.bias)] for a in members]

        def one_bank(table=start, count=n):
            clib.check(clib.lib.mm_policy_bank_act(obs.data_ptr(), count, S, ctypes.byref(bank.params), K, table, 128, A, 7,
                                                   ctr.data_ptr(), acts.data_ptr(), None, stream))

        def sequential():
            for k in range(K):
                lo, hi = start[k], start[k + 1]
                clib.check(clib.lib.mm_policy_act(obs.data_ptr() + 4 * S * lo, hi - lo, S, *w[k], 128, A, 7, ctr.data_ptr(),
                                                  acts.data_ptr() + 4 * lo, None, stream))

        def staging():
            one_bank(tiny, tiny[K])

        # the two variants agree before they are timed (same counter value: same draws)
        ctr.zero_(); one_bank(); a_bank = acts.clone()
        ctr.zero_(); sequential()
        lp_note = None
        if K == 1:
            assert torch.equal(a_bank, acts)
        else:  # the sequential calls key the sampler on the slice's own index: only the first group's draws coincide
            assert torch.equal(a_bank[:per], acts[:per])
            lp_note = "sequential calls key the sampler on slice-local indices"
        t = alternate({"bank": one_bank, "sequential": sequential, "staging": staging}, args.windows, args.reps)
        b, s, g = stats(t["bank"]), stats(t["sequential"]), stats(t["staging"])
        spread = max(b["spread_ms"], s["spread_ms"])
        rows.append({"agents": n, "K": K, "n_s": S, "n_a": A, "grid": int(grid[K]), "workgroups_per_group": wg[0],
                     "bank_launch": b, "sequential_mm_policy_act": s,
                     "difference_ms": s["mean_ms"] - b["mean_ms"], "larger_spread_ms": spread,
                     "bank_faster_by_more_than_spread": bool(s["mean_ms"] - b["mean_ms"] > spread),
                     "bank_slower_by_more_than_twice_spread": bool(b["mean_ms"] - s["mean_ms"] > 2 * spread),
                     "bank_ns_per_agent": b["mean_ms"] * 1e6 / n, "sequential_ns_per_agent": s["mean_ms"] * 1e6 / n,
                     "staged_KB": int(grid[K]) * 84, "staging_launch": g, "staging_share": g["mean_ms"] / b["mean_ms"],
                     "note": lp_note})
        print(json.dumps({k: v for k, v in rows[-1].items() if not isinstance(v, dict)}))
        del members, bank, obs, acts
    res = {"windows": args.windows, "reps": args.reps, "device": torch.cuda.get_device_name(0), "shapes": rows}
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
