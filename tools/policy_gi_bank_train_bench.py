#!/usr/bin/env python3
"""Timing of one train() of the K shared actor-critic members of a policy bank on a [T, E, N, S] rollout batch, T 100, N 8,
n_s 30, n_a 5, K equal env groups, form "reference" (N agent steps):

  (a) SharedBankPPOLearner.train(): per agent step two mm_policy_gi_bank_eval, one mm_policy_gi_bank_train, one mm_opt_step_bank;
  (b) what it replaces: K SharedPPOLearner(fused_step=True).train() calls, one after another, on the slices batch[:, group k].

    python tools/policy_gi_bank_train_bench.py [--json profiles/policy_gi_bank_train/bench.json] [--shapes 4096x16,512x64]

Shapes (E, K): (4096, 16), (65536, 16), (65536, 1), (512, 64).  One process; every shape is warmed up (one window of both
variants), then `windows` windows of `reps` back-to-back train() calls per variant, the two variants ALTERNATING window by
window.  Per window two figures per train(): the device time between two events around the calls, and the host time until the
calls have returned (enqueue only: nothing is synchronised inside a window; with several calls per window it includes waiting
for queue space) -- (b) issues its launches K times per agent step
and pays for them on the host too.  Beside every mean stand the lowest and the highest window and their difference (the spread);
`bank_faster_by_more_than_spread` compares the difference of the means with the larger of the two spreads.  `reps` is chosen per
shape so that a window of the slower variant takes about half a second, at most 10.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from marl_mass_amd import hip_library  # noqa: E402
from marl_mass_amd.learner import SharedBankPPOLearner, SharedPPOLearner  # noqa: E402
from marl_mass_amd.rollout import ActorCriticNetwork  # noqa: E402

T, N, S, A = 100, 8, 30, 5
SHAPES = ((4096, 16), (65536, 16), (65536, 1), (512, 64))


def window(fn, reps):
    """(device ms, host enqueue ms) per call of one window."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    h0 = time.perf_counter()
    for _ in range(reps):
        fn()
    h1 = time.perf_counter()
    t1.record(); t1.synchronize()
    return t0.elapsed_time(t1) / reps, (h1 - h0) * 1e3 / reps


def stats(w):
    return {"mean_ms": sum(w) / len(w), "min_ms": min(w), "max_ms": max(w), "spread_ms": max(w) - min(w), "windows_ms": w}


def compare(a, b):
    spread = max(a["spread_ms"], b["spread_ms"])
    return {"difference_ms": b["mean_ms"] - a["mean_ms"], "larger_spread_ms": spread,
            "bank_faster_by_more_than_spread": bool(b["mean_ms"] - a["mean_ms"] > spread),
            "bank_slower_by_more_than_spread": bool(a["mean_ms"] - b["mean_ms"] > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default=None, help="comma-separated ExK, default all")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    shapes = SHAPES if not args.shapes else tuple(tuple(int(v) for v in s.split("x")) for s in args.shapes.split(","))
    clib = hip_library()
    clib.require_policy_gi_bank_train()
    rows = []
    for E, K in shapes:
        torch.manual_seed(0)
        per = E // K
        groups = [per] * K
        members = [ActorCriticNetwork(S, A, 128, 1, state_split=True).cuda() for _ in range(K)]
        singles = [SharedPPOLearner(ActorCriticNetwork(S, A, 128, 1, state_split=True).cuda(), clib, fused_step=True) for _ in range(K)]
        bank = SharedBankPPOLearner(members, clib, groups)
        batch = {"states": torch.randn(T, E, N, S, device="cuda"),
                 "actions": torch.randint(0, A, (T, E, N), dtype=torch.int32, device="cuda"),
                 "returns": torch.randn(T, E, N, device="cuda")}
        parts = [{k: v[:, g * per:(g + 1) * per] for k, v in batch.items()} for g in range(K)]

        def bank_train():
            bank.train(batch, n_episodes=5)

        def sequential():
            for g in range(K):
                singles[g].train(parts[g], n_episodes=5)

        fns = {"bank": bank_train, "sequential": sequential}
        for fn in fns.values():  # (allocates every scratch)
            window(fn, 1)
        first = {k: window(fn, 1) for k, fn in fns.items()}
        slow = max(v[0] for v in first.values())
        reps = max(1, min(10, int(500.0 / slow)))
        for fn in fns.values():  # the warm-up window
            window(fn, reps)
        dev, host = {k: [] for k in fns}, {k: [] for k in fns}
        for _ in range(args.windows):
            for k, fn in fns.items():
                d, h = window(fn, reps)
                dev[k].append(d); host[k].append(h)
        d = {k: stats(v) for k, v in dev.items()}
        h = {k: stats(v) for k, v in host.items()}
        rows.append({"E": E, "K": K, "T": T, "N": N, "n_s": S, "n_a": A, "samples_per_member_and_agent_step": T * per,
                     "form": "reference", "reps": reps,
                     "device": {"bank_train": d["bank"], "sequential_shared_ppo_learners": d["sequential"], **compare(d["bank"], d["sequential"])},
                     "host_enqueue": {"bank_train": h["bank"], "sequential_shared_ppo_learners": h["sequential"],
                                      **compare(h["bank"], h["sequential"])}})
        r = rows[-1]
        print(json.dumps({"E": E, "K": K, "reps": reps,
                          "device_ms": [round(d["bank"]["mean_ms"], 3), round(d["sequential"]["mean_ms"], 3)],
                          "device_spread_ms": r["device"]["larger_spread_ms"], "device_bank_faster": r["device"]["bank_faster_by_more_than_spread"],
                          "host_ms": [round(h["bank"]["mean_ms"], 3), round(h["sequential"]["mean_ms"], 3)]}), flush=True)
        del bank, singles, batch, parts, members
        torch.cuda.empty_cache()
    res = {"windows": args.windows, "device": torch.cuda.get_device_name(0), "shapes": rows}
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
