#!/usr/bin/env python3
"""Timing of the shared-policy bank's act launch on the device (include/mm_policy_gi_bank.h), n_s 30, n_a 5, K equal groups of
state-split hidden-128 ActorCriticNetworks:

  (a) `bank`: ONE mm_policy_gi_bank_act launch over the whole batch (+ its counter bump);
  (b) `sequential`: K mm_policy_gi_act calls on the groups' slices (K launches + K counter bumps);
  (c) `modules`: what DeviceRollout's bank mode did for such members before the entry existed: K torch module forwards into one
      log-probability buffer + ONE mm_sample_actions;
and the bootstrap's draw + value: `bank_value` (the same launch with the value output) against `sequential_value` (K
mm_policy_gi_act calls with actions and value, as DeviceRollout._policy_gi makes one).

    python tools/policy_gi_bank_bench.py [--json profiles/policy_gi_bank/bench.json]

Shapes and protocol are tools/policy_bank_bench.py's: 524 288 agents with K in {1, 4, 16, 64} and 32 768 agents with K = 16 (the
population case, in which launches dominate); device time from events; every shape is warmed up (one window of every variant),
then `windows` windows of `reps` back-to-back calls per variant, the variants ALTERNATING window by window in the same process.
Beside every mean stand the lowest and the highest window and their difference (the spread); a `..._by_more_than_spread` flag
compares the difference of two means with the larger of the two spreads.
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402
from marl_mass_amd import hip_library  # noqa: E402
from marl_mass_amd.rollout import ActorCriticNetwork, SharedPolicyBank  # noqa: E402
from policy_bank_bench import SHAPES, alternate, stats  # noqa: E402

S, A = 30, 5


def versus(a, b):
    """a against baseline b: the difference of the means, the larger spread, and on which side of it the difference falls."""
    spread = max(a["spread_ms"], b["spread_ms"])
    diff = b["mean_ms"] - a["mean_ms"]
    return {"difference_ms": diff, "larger_spread_ms": spread, "speedup": b["mean_ms"] / a["mean_ms"],
            "faster_by_more_than_spread": bool(diff > spread), "slower_by_more_than_spread": bool(-diff > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    clib = hip_library()
    clib.require_policy_gi_bank()
    torch.manual_seed(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    rows = []
    for n, K in SHAPES:
        members = [ActorCriticNetwork(S, A, 128, 1, state_split=True).cuda() for _ in range(K)]
        bank = SharedPolicyBank(members)
        obs = torch.randn(n, S, device="cuda").contiguous()
        acts = torch.empty(n, dtype=torch.int32, device="cuda")
        val = torch.empty(n, dtype=torch.float32, device="cuda")
        logp = torch.empty(n, A, dtype=torch.float32, device="cuda")
        per = n // K
        start = (ctypes.c_int64 * (K + 1))(*[k * per for k in range(K)] + [n])
        grid = (ctypes.c_int32 * (K + 1))()
        clib.check(clib.lib.mm_policy_bank_grid(K, start, grid))
        w = [[p.detach().data_ptr() for p in SharedPolicyBank._params(m)] for m in members]

        def one_bank(value=None):
            clib.check(clib.lib.mm_policy_gi_bank_act(obs.data_ptr(), n, S, ctypes.byref(bank.params), K, start, 128, A, 7,
                                                      ctr.data_ptr(), acts.data_ptr(), None, value, stream))

        def sequential(value=None):
            for k in range(K):
                lo, hi = start[k], start[k + 1]
                clib.check(clib.lib.mm_policy_gi_act(obs.data_ptr() + 4 * S * lo, hi - lo, S, *w[k], 128, A, 7, ctr.data_ptr(),
                                                     acts.data_ptr() + 4 * lo, None, None if value is None else value + 4 * lo,
                                                     stream))

        @torch.no_grad()
        def modules():
            for k in range(K):
                logp[start[k]:start[k + 1]] = members[k](obs[start[k]:start[k + 1]])
            clib.check(clib.lib.mm_sample_actions(logp.data_ptr(), n, A, 7, ctr.data_ptr(), acts.data_ptr(), stream))

        def bank_value():
            one_bank(val.data_ptr())

        def sequential_value():
            sequential(val.data_ptr())

        # the variants agree before they are timed (same counter value: same draws)
        ctr.zero_(); bank_value(); a_bank, v_bank = acts.clone(), val.clone()
        ctr.zero_(); sequential_value()
        assert torch.equal(v_bank, val)  # bit for bit
        assert torch.equal(a_bank[:per], acts[:per])  # (the slices' calls key the sampler on slice-local indices)
        ctr.zero_(); modules()
        agree = float((a_bank == acts).float().mean())  # the modules' float32 rows may move a draw at a CDF edge
        assert agree > 0.999, agree
        t = alternate({"bank": one_bank, "sequential": sequential, "modules": modules, "bank_value": bank_value,
                       "sequential_value": sequential_value}, args.windows, args.reps)
        st = {k: stats(v) for k, v in t.items()}
        row = {"agents": n, "K": K, "n_s": S, "n_a": A, "grid": int(grid[K]), "workgroups_per_group": int(grid[1] - grid[0]),
               "bank_launch": st["bank"], "sequential_mm_policy_gi_act": st["sequential"], "module_forwards_plus_sample": st["modules"],
               "bank_vs_sequential": versus(st["bank"], st["sequential"]), "bank_vs_modules": versus(st["bank"], st["modules"]),
               "bank_draw_and_value": st["bank_value"], "sequential_draw_and_value": st["sequential_value"],
               "bank_vs_sequential_draw_and_value": versus(st["bank_value"], st["sequential_value"]),
               "bank_ns_per_agent": st["bank"]["mean_ms"] * 1e6 / n, "modules_agree_share": agree}
        rows.append(row)
        print(json.dumps({"agents": n, "K": K, "bank_ms": st["bank"]["mean_ms"], "sequential_ms": st["sequential"]["mean_ms"],
                          "modules_ms": st["modules"]["mean_ms"], "bank_value_ms": st["bank_value"]["mean_ms"],
                          "sequential_value_ms": st["sequential_value"]["mean_ms"],
                          "vs_sequential": row["bank_vs_sequential"], "vs_modules": row["bank_vs_modules"]}), flush=True)
        del members, bank, obs, acts, val, logp
    res = {"windows": args.windows, "reps": args.reps, "device": torch.cuda.get_device_name(0), "shapes": rows}
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
