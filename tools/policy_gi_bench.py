#!/usr/bin/env python3
"""Timing of MAPPO_GI's shared actor-critic on the device (include/mm_policy_gi.h), at E envs x 8 agents, n_s 30:

  * mm_policy_gi_act alone (forward + sample, one launch + the counter bump);
  * the torch path DeviceRollout takes without the fused entry: ActorCriticNetwork forward + mm_sample_actions;
  * DeviceRollout.interact() in shared mode, eager and hipGraph-replayed (T policy steps of the MASS-shielded v1 env).

    python tools/policy_gi_bench.py [E] [--json out.json]

Device times from CUDA events over `reps` back-to-back calls after a warm-up; rollouts from the wall clock after a
synchronise (they include the host's launch overhead, which is what the graph removes).
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
from marl_mass_amd.rollout import ActorCriticNetwork, DeviceRollout  # noqa: E402


def device_ms(fn, reps=50):
    fn(); torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record(); t1.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("E", nargs="?", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    E, N, S, T = args.E, 8, 30, args.steps
    kw = dict(config={"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}, cbf_eta=0.03125, qp_solver="exact", cbf_tau=0.5, seed=9,
              auto_reset=True)
    torch.manual_seed(0)
    net = ActorCriticNetwork(S, 5, 128, 1, state_split=True).cuda()
    clib = hip_library()
    n = E * N
    obs = torch.randn(n, S, device="cuda").contiguous()
    acts = torch.empty(n, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: t.detach().contiguous().data_ptr()  # noqa: E731
    w = [p(t) for t in (net.fc11.weight, net.fc11.bias, net.fc12.weight, net.fc12.bias, net.fc13.weight, net.fc13.bias,
                        net.fc2.weight, net.fc2.bias, net.actor_linear.weight, net.actor_linear.bias, net.critic_linear.weight,
                        net.critic_linear.bias)]

    def fused():
        clib.check(clib.lib.mm_policy_gi_act(obs.data_ptr(), n, S, *w, 128, 5, 7, ctr.data_ptr(), acts.data_ptr(), None, None, stream))

    def torch_path():
        with torch.no_grad():
            lp = net(obs).contiguous()
        clib.check(clib.lib.mm_sample_actions(lp.data_ptr(), n, 5, 7, ctr.data_ptr(), acts.data_ptr(), stream))

    res = {"E": E, "N": N, "n_s": S, "agents": n,
           "mm_policy_gi_act_ms": device_ms(fused), "torch_forward_plus_sample_ms": device_ms(torch_path)}
    for graph in (False, True):
        ro = DeviceRollout(VecMergeEnv(E, N, **kw), net, roll_out_n_steps=T, use_graph=graph)
        assert ro.shared and ro.fused_policy
        ro.interact(); ro.interact(); torch.cuda.synchronize()
        t0 = time.perf_counter(); ro.interact(); ro.interact(); torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 2
        res["interact_%s_ms_per_step" % ("graph" if graph else "eager")] = dt * 1e3 / T
    res["steps"] = T
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
