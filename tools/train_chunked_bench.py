#!/usr/bin/env python3
"""Timing of the chunked gradient entries (mm_policy_gi_train_chunked / mm_policy_train_chunked, and with --entry wide
mm_policy_wide_train_chunked: the separate networks at hidden 512) on the device, n_s 30:

  * the chunked call on n = passes x chunk samples (default 4 x 524 288) against the unchunked entry called on the same
    `passes` parts one after the other, in the same run and in alternating windows: the A and B work is the same, the chunked
    call runs one accumulate per pass where each separate call runs one fold, and one prep instead of `passes`;
  * one agent step of train(form="reference") at n = --step-n samples (default 6 553 600: 65 536 envs x 100 steps) with a
    learner under --budget-gib of scratch (default 2), which the unchunked entry cannot run at all within that budget.

    python tools/train_chunked_bench.py [--entry gi|pt|wide|both] [--chunk 524288] [--passes 4] [--step-n 6553600] [--json out.json]

"both" is gi and pt, the two hidden-128 entries.  A hidden-512 call takes about nine times as long: --entry wide --reps 10
--step-reps 4 is what profiles/wide_chunked/bench.json was taken with.
--step-n 0 leaves the agent step out: under `rocprofv3 --kernel-trace --stats` that run gives the accumulate and the fold
kernels' own times side by side.

Device time by events, 5 windows each after a warm-up.  The separate calls write the gradient of their own part; only their
time is compared (that the chunked call computes the gradient of the whole batch is tests/test_train_chunked_gpu.py).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from marl_mass_amd import hip_library  # noqa: E402
from marl_mass_amd.learner import PPOLearner, SharedPPOLearner  # noqa: E402
from marl_mass_amd.rollout import ActorCriticNetwork, ActorNetwork, CriticNetwork  # noqa: E402

S, N_A = 30, 5


def alternating_ms(fns, reps, windows=5):
    """Device time per call of each function by events: `windows` rounds, in each one window of `reps` back-to-back calls per
    function, the functions taking turns; per function (mean, lowest window, highest window)."""
    for fn in fns:
        fn(); fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn()
            t1.record(); t1.synchronize()
            out[i].append(t0.elapsed_time(t1) / reps)
    return [(sum(o) / windows, min(o), max(o)) for o in out]


def make_learner(entry, clib, **kw):
    torch.manual_seed(0)
    if entry == "gi":
        net = ActorCriticNetwork(S, N_A, 128, 1, state_split=True).cuda()
        learner, nets = SharedPPOLearner(net, clib, **kw), [net]
    else:
        hidden = 512 if entry == "wide" else 128
        actor, critic = ActorNetwork(S, hidden, N_A).cuda(), CriticNetwork(S, N_A, hidden, 1).cuda()
        learner, nets = PPOLearner(actor, critic, clib, **kw), [actor, critic]
    with torch.no_grad():  # networks that have moved away from their targets: ratios off 1
        for net in nets:
            for p in net.parameters():
                p.add_(0.01 * torch.randn_like(p))
    return learner


def batch(n):
    g = torch.Generator(device="cuda").manual_seed(1)
    obs = torch.randn(n, S, device="cuda", generator=g)
    act = torch.randint(0, N_A, (n,), device="cuda", generator=g, dtype=torch.int32)
    ret = torch.randn(n, device="cuda", generator=g)
    return obs, act, ret


def queries(entry, clib):
    """(chunked, unchunked) size queries of the entry."""
    return {"gi": (clib.policy_gi_train_chunked_scratch_bytes, clib.policy_gi_train_scratch_bytes),
            "pt": (clib.policy_train_chunked_scratch_bytes, clib.policy_train_scratch_bytes),
            "wide": (clib.policy_wide_train_chunked_scratch_bytes, clib.policy_wide_train_scratch_bytes)}[entry]


def inputs(entry, learner, obs, act, ret):
    """(old_logp, keyword arguments of loss_and_grad) for the reference form."""
    if entry == "gi":
        return learner.old_log_probs(obs, act), dict(adv_sums=learner.advantage_sums(obs, ret))
    old, value = learner.evaluate(obs, act, actor=learner.actor_target, critic=learner.critic_target)
    adv = ret - value
    return old, dict(adv_sums=torch.stack([adv.clamp(min=0).sum(), adv.clamp(max=0).sum()]))


def compare(entry, clib, chunk, passes, reps):
    n = chunk * passes
    obs, act, ret = batch(n)
    whole = make_learner(entry, clib)  # no budget: the unchunked entry, called on the parts
    query, unchunked = queries(entry, clib)
    budget = query(n, chunk)
    chunked = make_learner(entry, clib, scratch_budget_bytes=budget)  # exactly `passes` passes of `chunk`
    old, kw = inputs(entry, whole, obs, act, ret)
    parts = [slice(q * chunk, (q + 1) * chunk) for q in range(passes)]

    def separate_calls():
        for p in parts:
            whole.loss_and_grad(obs[p], act[p], ret[p], old[p], **kw)

    def chunked_call():
        chunked.loss_and_grad(obs, act, ret, old, **kw)

    (sep, sep_lo, sep_hi), (chk, chk_lo, chk_hi) = alternating_ms([separate_calls, chunked_call], reps)
    assert chunked._plan(n)[0] == chunk and chunked._scratch.numel() <= budget
    return {"n": n, "chunk": chunk, "passes": passes, "reps_per_window": reps,
            "separate_calls_ms": sep, "separate_calls_ms_min": sep_lo, "separate_calls_ms_max": sep_hi,
            "chunked_ms": chk, "chunked_ms_min": chk_lo, "chunked_ms_max": chk_hi, "chunked_over_separate": chk / sep,
            "chunked_scratch_MB": budget / 2 ** 20, "unchunked_scratch_of_n_MB": unchunked(n) / 2 ** 20}


def agent_step(entry, clib, n, budget, reps):
    obs, act, ret = batch(n)
    learner = make_learner(entry, clib, scratch_budget_bytes=budget)

    def step():
        learner.train(obs.view(n, 1, S), act.view(n, 1), ret.view(n, 1), n_episodes=0)

    (ms, lo, hi), = alternating_ms([step], reps)
    chunk = learner._plan(n)[0]
    unchunked = queries(entry, clib)[1]
    return {"n": n, "budget_MB": budget / 2 ** 20, "chunk": chunk, "passes": None if chunk is None else -(-n // chunk),
            "scratch_MB": learner._scratch.numel() / 2 ** 20, "unchunked_scratch_of_n_MB": unchunked(n) / 2 ** 20,
            "reps_per_window": reps, "train_reference_agent_step_ms": ms, "train_reference_agent_step_ms_min": lo,
            "train_reference_agent_step_ms_max": hi, "samples_per_s": n / ms * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entry", default="both", choices=["gi", "pt", "wide", "both"])
    ap.add_argument("--chunk", type=int, default=524288)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--step-n", type=int, default=6553600)
    ap.add_argument("--budget-gib", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    clib = hip_library()
    res = {"n_s": S, "n_a": N_A, "device": torch.cuda.get_device_name(0)}
    for entry in (("gi", "pt") if args.entry == "both" else (args.entry,)):
        res[entry] = {"chunked_vs_separate_calls": compare(entry, clib, args.chunk, args.passes, args.reps)}
        if args.step_n > 0:
            res[entry]["agent_step_under_budget"] = agent_step(entry, clib, args.step_n, int(args.budget_gib * 2 ** 30),
                                                               args.step_reps)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
