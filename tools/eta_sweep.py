#!/usr/bin/env python3
"""The reference's eta search (test/cbf/eta_binary_search.sh: one whole run per value) as ONE batch.

    python tools/eta_sweep.py [--actor CHECKPOINT.pt] [--seeds 64] [--N 8] [--out profiles/env_params/eta_sweep.json]

merge-multi-agent-v1, MASS, N CAVs.  Grid: the script's six eta values x HEADWAY_TIME {0.5, 1.2} (the two .ini files; cbf_tau
follows HEADWAY_TIME as run_mappo.py:138-139 sets it) x `seeds` evaluation seeds = one batch of 12 * seeds envs, every env
with its own cbf_eta / cbf_tau / HEADWAY_TIME (VecMergeEnv(env_params=...)), one DeviceRollout.evaluate() for all of it and
rollout.group_ext_info for the per-point means.  --actor: a state_dict of the reference's ActorNetwork (fc1 / fc2 / fc3);
without it the policy is uniform-random (an actor with zero weights: equal logits).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from marl_mass_amd import VecMergeEnv  # noqa: E402
from marl_mass_amd.rollout import ActorNetwork, DeviceRollout, group_ext_info  # noqa: E402

ETAS = (0.5, 0.25, 0.125, 0.0625, 0.03125, 0.046875)  # eta_binary_search.sh, in its order
HEADWAY_TIMES = (0.5, 1.2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actor", default=None)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--qp-solver", choices=("exact", "ipm"), default="ipm")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "env_params", "eta_sweep.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eta_sweep.py runs on the GPU: none found")
    points = [(eta, ht) for ht in HEADWAY_TIMES for eta in ETAS]
    E = len(points) * a.seeds
    groups = torch.arange(E) // a.seeds  # env e: grid point e // seeds, evaluation seed e % seeds
    eta = torch.tensor([p[0] for p in points], dtype=torch.float64)[groups]
    ht = torch.tensor([p[1] for p in points], dtype=torch.float64)[groups]
    env = VecMergeEnv(E, a.N, config={"safety_guarantee": "cbf-cav", "HEADWAY_TIME": HEADWAY_TIMES[0]}, cbf_eta=ETAS[0], seed=0,
                      qp_solver=a.qp_solver, env_params={"cbf_eta": eta, "cbf_tau": ht, "HEADWAY_TIME": ht})
    if a.actor:
        sd = torch.load(a.actor, map_location="cpu")
        actor = ActorNetwork(env.n_s, sd["fc2.weight"].shape[0], env.n_a)
        actor.load_state_dict(sd)
        policy = os.path.basename(a.actor)
    else:
        actor = ActorNetwork(env.n_s, 128, env.n_a)
        for p in actor.parameters():
            torch.nn.init.zeros_(p)
        policy = "uniform-random"
    ro = DeviceRollout(env, actor.to(env.device), roll_out_n_steps=env.T)
    seeds = (torch.arange(E) % a.seeds).tolist()  # the same seeds at every grid point
    _, _, ext = ro.evaluate(seeds=seeds)
    env.poll_errors()
    g = group_ext_info(ext, groups.to(env.device), n_groups=len(points))
    rows = []
    for k, (e_, h_) in enumerate(points):
        rows.append({"cbf_eta": e_, "cbf_tau": h_, "HEADWAY_TIME": h_, "episodes": int(g["count"][k]),
                     **{key: float(g[key][k]) for key in ("steps", "avg_speeds", "crash_rate", "traffic_speeds", "merge_percents")}})
    res = {"env": "merge-multi-agent-v1", "shield": "MASS", "N": a.N, "qp_solver": a.qp_solver, "policy": policy, "seeds": a.seeds,
           "envs": E, "launches_per_step": 1, "min_headway_all": ext["min_headway"], "points": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
