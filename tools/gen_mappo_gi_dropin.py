#!/usr/bin/env python3
"""Drop-in fixtures of the reference's shared actor-critic learner (build container only; the reference cannot travel).

The companion of tools/gen_mappo_dropin.py for MAPPO_GI with shared_network = True (marl/mappo_gi.py, the learner of the
"*-shared" configs; network Model_gi.ActorCriticNetwork(state_split=True)).  Imports the reference's marl/mappo_gi.py
under the stand-ins of tools/refshim, drives `MAPPO_GI.interact()` x 6 (roll_out_n_steps 40) and `MAPPO_GI.evaluation()`
on the test seeds [0, 25, 50] with the env configured as run_mappo.py does from the case's .ini, and writes what that
run produced (tests/golden/mappo_gi_*.npz):

  * the policy's weights (MAPPO_GI.save's `policy.state_dict()` keys fc11.* fc12.* fc13.* fc2.* actor_linear.*
    critic_linear.*), the states MAPPO_GI stored, the actions it took, the discounted returns it pushed to memory
    (with the shared critic's bootstrap), episode boundaries;
  * the policy's log-probabilities (out_type "p") and values (out_type "v") on those states;
  * evaluation(): rewards per step and ext_info.

Cases (marl/configs):
  v1mass  marl_cav-heading-t_headway-cbf-cav-mixed-srew-shared.ini   v1, cbf-cav, mixed traffic, srew, exact QP
  v1none  configs_marl-cav-heading-t_headway-shared-unsafe.ini       v1, no shield, CAVs only
  v0prio  marl_cav-heading-t_headway-priority-mixed-shared.ini       v0, "priority" supervisor, mixed traffic, density 3
For the v1 cases the SAME MAPPO_GI object code is first run on marl_mass_amd.compat.make(env_id) with the CPU oracle as
backend and must draw the identical action sequence and match states / returns / ext_info to 1e-9 before anything is
written.  The oracle had no supervisor when v0prio was recorded, so it comes from the reference alone (meta says so); the HIP backend
replays it in tests/test_mappo_gi_dropin.py.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_mappo_dropin as gmd  # noqa: E402  (puts the reference, the shims and this repo on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import gym  # noqa: E402
import cvxopt  # noqa: E402
from highway_env.vehicle.safety.cbf import CBFType as RefCBFType  # noqa: E402
from marl.mappo_gi import MAPPO_GI  # noqa: E402  (the reference's caller)

import oracle_env  # noqa: E402
from marl_mass_amd import compat  # noqa: E402

OUT = gmd.OUT
BASE = dict(simulation_frequency=15, duration=20, policy_frequency=5, action_masking=False)
# ENV_CONFIG / MODEL_CONFIG values of each .ini as run_mappo.py:137-171 writes them (fallbacks included)
CASES = {
    "v1mass": dict(ini="marl_cav-heading-t_headway-cbf-cav-mixed-srew-shared.ini", env_id="merge-multi-agent-v1", eta=0.03125,
                   check_dropin=True,
                   cfg=dict(COLLISION_REWARD=200, HIGH_SPEED_REWARD=4, HEADWAY_COST=1, HEADWAY_TIME=0.5, MERGING_LANE_COST=8,
                            traffic_density=1, safety_guarantee="cbf-cav", lateral_control="steer", mixed_traffic=True,
                            traffic_type="mixed", agent_reward="srew")),
    "v1none": dict(ini="configs_marl-cav-heading-t_headway-shared-unsafe.ini", env_id="merge-multi-agent-v1", eta=0.0,
                   check_dropin=True,
                   cfg=dict(COLLISION_REWARD=200, HIGH_SPEED_REWARD=1, HEADWAY_COST=4, HEADWAY_TIME=0.5, MERGING_LANE_COST=4,
                            traffic_density=1, safety_guarantee="none", lateral_control="steer", mixed_traffic=False,
                            traffic_type="cav", agent_reward="default")),
    "v0prio": dict(ini="marl_cav-heading-t_headway-priority-mixed-shared.ini", env_id="merge-multi-agent-v0", eta=0.0,
                   check_dropin=False,
                   cfg=dict(COLLISION_REWARD=200, HIGH_SPEED_REWARD=1, HEADWAY_COST=4, HEADWAY_TIME=0.5, MERGING_LANE_COST=4,
                            traffic_density=3, safety_guarantee="priority", lateral_control="steer", mixed_traffic=True,
                            traffic_type="mixed", agent_reward="default")),
}


def configure(env, cfg, seed):
    for k, v in dict(BASE, **cfg).items():
        env.config[k] = v
    env.config["seed"] = seed
    env.seed = seed
    if hasattr(env, "unwrapped"):
        env.unwrapped.seed = seed
    return env


def drive(make_env, case, K, T, test_seeds):
    """MAPPO_GI's training / evaluation calls, in run_mappo.py's order (:233-306)."""
    cfg, eta, tau = case["cfg"], case["eta"], case["cfg"]["HEADWAY_TIME"]
    RefCBFType.GAMMA_B, RefCBFType.TAU = eta, tau
    # the closed-form QP on both sides (the reference's cvxopt stand-in and the drop-in), as tools/gen_mappo_dropin.py
    compat.CBFType.GAMMA_B, compat.CBFType.TAU, compat.CBFType.QP_SOLVER = eta, tau, "exact"
    cvxopt.solvers.mode = "exact"
    env = configure(make_env(case["env_id"]), cfg, seed=0)
    env_eval = configure(make_env(case["env_id"]), cfg, seed=0)
    torch.manual_seed(1234)
    mappo = MAPPO_GI(env=env, state_dim=env.n_s, action_dim=env.n_a, memory_capacity=10000, roll_out_n_steps=T,
                     reward_gamma=0.99, reward_scale=20.0, use_cuda=False, traffic_density=cfg["traffic_density"],
                     reward_type="regionalR", shared_network=True, test_seeds=",".join(str(s) for s in test_seeds),
                     max_steps=None)
    rollouts = []
    for _ in range(K):
        n_before = len(mappo.memory.memory)
        mappo.interact()
        exps = mappo.memory.memory[n_before:]
        rollouts.append(dict(states=np.array([e.states for e in exps], dtype=np.float64),
                             actions=np.array([e.actions for e in exps], dtype=np.float64).argmax(-1).astype(np.int32),
                             returns=np.array([e.rewards for e in exps], dtype=np.float64),
                             episode_done=bool(mappo.episode_done), n_agents=int(mappo.n_agents)))
    rewards, (vspeed, vpos), ext = mappo.evaluation(env_eval, None, eval_episodes=len(test_seeds), is_train=False)
    weights = {k: v.numpy().copy() for k, v in mappo.policy.state_dict().items()}
    logp, values = [], []
    with torch.no_grad():
        for r in rollouts:
            s = torch.tensor(r["states"], dtype=torch.float32).reshape(-1, env.n_s)
            logp.append(mappo.policy(s).numpy().reshape(r["states"].shape[0], r["n_agents"], env.n_a))
            values.append(mappo.policy(s, out_type="v").numpy().reshape(r["states"].shape[0], r["n_agents"]))
    return dict(rollouts=rollouts, logp=logp, values=values, eval_rewards=[np.array(r, dtype=np.float64) for r in rewards],
                ext={k: (float(v) if np.isscalar(v) else [float(x) for x in v]) for k, v in ext.items() if k != "step_time"},
                weights=weights, n_s=int(env.n_s), n_a=int(env.n_a))


def main():
    os.makedirs(OUT, exist_ok=True)
    only = sys.argv[1:] or list(CASES)
    for tag in only:
        case = CASES[tag]
        K, T, test_seeds = 6, 40, [0, 25, 50]
        ref = drive(lambda eid: gym.make(eid), case, K, T, test_seeds)
        if case["check_dropin"]:
            dropin = drive(lambda eid: compat.make(eid, backend_factory=lambda **kw: oracle_env.OracleEnv(**kw)), case, K, T,
                           test_seeds)
            worst = gmd.compare(ref, dropin)
            assert worst <= 1e-9, worst
            note = ("recorded from the reference's MAPPO_GI (shared_network=True) on the reference env; at generation time the "
                    "same MAPPO_GI on marl_mass_amd.compat (oracle backend) drew the identical action sequence and matched to "
                    "%.1e" % worst)
        else:
            worst = None
            note = ("recorded from the reference's MAPPO_GI (shared_network=True) on the reference env only: the CPU oracle "
                    "has no 'priority' supervisor, so there was no drop-in cross-check at generation time; the HIP backend "
                    "replays this run in tests/test_mappo_gi_dropin.py")
        meta = dict(env_id=case["env_id"], ini=case["ini"], shield=case["cfg"]["safety_guarantee"],
                    headway_time=case["cfg"]["HEADWAY_TIME"], eta=case["eta"], qp_solver="exact", K=K, roll_out_n_steps=T, test_seeds=test_seeds,
                    torch_seed=1234, env_seed=0, reward_type="regionalR", reward_scale=20.0, reward_gamma=0.99,
                    n_s=ref["n_s"], n_a=ref["n_a"], hidden=128, state_split=True, env_config=dict(BASE, **case["cfg"]),
                    dropin_checked=case["check_dropin"], dropin_vs_reference_max_abs=worst, note=note)
        arrays = {}
        for k, r in enumerate(ref["rollouts"]):
            arrays["ro%d_states" % k], arrays["ro%d_actions" % k], arrays["ro%d_returns" % k] = r["states"], r["actions"], r["returns"]
            arrays["ro%d_logp" % k] = ref["logp"][k].astype(np.float32)
            arrays["ro%d_value" % k] = ref["values"][k].astype(np.float32)
            arrays["ro%d_done" % k] = np.array(r["episode_done"])
        for k, r in enumerate(ref["eval_rewards"]):
            arrays["ev%d_rewards" % k] = r
        for k, v in ref["weights"].items():
            arrays["w_" + k] = v
        path = os.path.join(OUT, "mappo_gi_%s.npz" % tag)
        np.savez_compressed(path, meta=json.dumps(meta), ext=json.dumps(ref["ext"]), **arrays)
        size = os.path.getsize(path)
        assert size <= 500 * 1024, (path, size)
        print("%-7s %s %s: %d rollouts (agents %s), eval steps %s, drop-in %s, %d bytes"
              % (tag, case["env_id"], case["cfg"]["safety_guarantee"], K, [r["n_agents"] for r in ref["rollouts"]],
                 ref["ext"]["steps"], "== reference to %.2e" % worst if worst is not None else "not checked (no oracle twin)", size))


if __name__ == "__main__":
    main()
