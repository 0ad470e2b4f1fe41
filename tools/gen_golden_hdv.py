#!/usr/bin/env python3
"""Golden tapes of the reference's all-HDV baseline env merge-multi-agent-hdv-v1 (runs in the build container only).

Imports the reference under tools/refshim exactly as tools/gen_golden.py does, runs MergeEnvLCHDV (merge_env_v1.py:552-674)
with env.step(None) the way eval_idm.py:70-160 does and records what the device path is checked against.  The outputs are
DATA only (tests/golden/idm_*.npz, idm_index.json, idm_reset.json); the prefix idm_ keeps them out of
golden_util.episode_files.

    python tools/gen_golden_hdv.py

Per tape (m vehicles, all IDMVehicleHist): meta (json: density, HEADWAY_TIME, seed or placement, and `eval`, the episode's
eval_idm.py results); init_f [m][4] the spawn (x, y, heading, speed); reset_obs [m][30]; for the whole episode rewards,
dones, sub_count [T] and info_f [T][5] (speed, crashed of vehicle 0, average_speed, traffic_speed, min_headway),
merge_percent [T] (NaN unless terminal), end_f / end_i [T][m] the state of every vehicle at the end of every step (columns
of gen_golden._veh_snapshot: what teacher forcing starts the next step from); for the first K = 20 steps (size) sub_f /
sub_i, the same after every sub-step, and obs [K][m][30].
idm_reset.json: the vehicle-count support and the spawn draws of reset(is_training=False, testing_seeds=s) per density.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (puts the reference and the shims on sys.path)
import gym  # noqa: E402
import numpy as np  # noqa: E402

OUT = gg.OUT
K = 20  # steps with per-sub-step state and observations (keeps a tape below ~100 KB)
ENV_ID = "merge-multi-agent-hdv-v1"


def make_env(density, headway_time):
    """eval_idm.py's configuration (simulation 15 Hz, policy 5 Hz, 20 s) with the reward constants of the .ini files."""
    env = gym.make(ENV_ID)
    for k, v in (("simulation_frequency", 15), ("duration", 20), ("policy_frequency", 5), ("COLLISION_REWARD", 200),
                 ("HIGH_SPEED_REWARD", 1), ("HEADWAY_COST", 4), ("HEADWAY_TIME", headway_time), ("MERGING_LANE_COST", 4),
                 ("traffic_density", density)):
        env.config[k] = v
    return env


def run_tape(name, density, headway_time, seed=None, placement=None):
    env = make_env(density, headway_time)
    obs0, avail = env.reset(is_training=False, testing_seeds=0 if seed is None else seed)
    assert np.shape(avail) == (0,)
    if placement is not None:
        obs0 = gg._place_vehicles(env, placement)
    vs = env.road.vehicles
    init = [[v.position[0], v.position[1], v.heading, v.speed] for v in vs]
    gg._SUBSTEP_LOG = []
    rewards, dones, counts, info_f, merge, obs = [], [], [], [], [], []
    done, step, avg_speed, traffic_speed, min_hw = False, 0, 0.0, None, float("inf")
    while not done:
        before = len(gg._SUBSTEP_LOG)
        o, r, done, info = env.step(None)
        step += 1
        counts.append(len(gg._SUBSTEP_LOG) - before)
        rewards.append(r)
        dones.append(done)
        info_f.append([info["speed"], float(info["crashed"]), info["average_speed"], info["traffic_speed"], info["min_headway"]])
        merge.append(info.get("merge_percent", np.nan))
        if step <= K:
            obs.append(np.asarray(o, dtype=np.float64).reshape(len(vs), -1))
        avg_speed += info["average_speed"]  # eval_idm.py:124-129
        min_hw = max(0, min(min_hw, info["min_headway"]))
        traffic_speed = info["traffic_speed"] if traffic_speed is None else traffic_speed + info["traffic_speed"]
    log, gg._SUBSTEP_LOG = gg._SUBSTEP_LOG, None
    S = sum(counts[:K])
    ends = np.cumsum(counts) - 1
    ev = dict(steps=step, avg_speed=avg_speed / step, crashed=bool(env.is_crashed()), min_headway=min_hw,
              traffic_speed=traffic_speed / step, merge_percent=merge[-1])
    meta = dict(env_id=ENV_ID, n=0, n_hdv=len(vs), headway_time=headway_time, density=density, seed=seed,
                placement=placement, n_merge=int(env.n_merge), steps=step, K=min(K, step), eval=ev)
    z = dict(init_f=np.array(init, dtype=np.float64), reset_obs=np.asarray(obs0, dtype=np.float64).reshape(len(vs), -1),
             rewards=np.array(rewards, dtype=np.float64), dones=np.array(dones, dtype=np.uint8),
             sub_count=np.array(counts, dtype=np.int32), info_f=np.array(info_f, dtype=np.float64),
             merge_percent=np.array(merge, dtype=np.float64), obs=np.array(obs),
             sub_f=np.array([r[0] for r in log[:S]]), sub_i=np.array([r[1] for r in log[:S]], dtype=np.int32),
             end_f=np.array([log[k][0] for k in ends]), end_i=np.array([log[k][1] for k in ends], dtype=np.int32))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, meta=json.dumps(meta), **z)
    crashed = int(np.array([r[1][:, 3] for r in log]).any())
    print("%-30s m=%2d T=%3d crashed=%d  %5.1f KB" % (name, len(vs), step, crashed, os.path.getsize(path) / 1024))
    return dict(name=name, m=len(vs), steps=step, crashed=bool(crashed), density=density, headway_time=headway_time)


def gen_reset():
    """Count support and spawn draws of reset(is_training=False, testing_seeds=s) (merge_env_v1.py:180-211,490-494,265-364)."""
    out = {}
    for density in (1, 2, 3):
        env = make_env(density, 1.2)
        counts, spawns = {}, []
        for s in range(300):
            env.reset(is_training=False, testing_seeds=s)
            m = len(env.road.vehicles)
            counts[m] = counts.get(m, 0) + 1
            if s < 20:
                spawns.append(dict(seed=s, x=[float(v.position[0]) for v in env.road.vehicles],
                                   y=[float(v.position[1]) for v in env.road.vehicles],
                                   speed=[float(v.speed) for v in env.road.vehicles]))
        out[str(density)] = dict(counts={str(k): v for k, v in sorted(counts.items())}, spawns=spawns)
    with open(os.path.join(OUT, "idm_reset.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("idm_reset.json:", {d: out[d]["counts"] for d in out})


def main():
    index = []
    for density in (1, 2, 3):
        for ht in (1.2, 0.5):
            for seed in (3 + 10 * density, 7 + 10 * density):
                index.append(run_tape("idm_d%d_ht%s_s%d" % (density, str(ht).replace(".", ""), seed), density, ht, seed=seed))
    # placed scenarios (random seeds did not crash): rows (x, y, speed, heading, "h") in creation order
    index.append(run_tape("idm_placed_obstacle", 1, 1.2, placement=[(100, 0.0, 25, 0.0, "h"), (404, 4.0, 24, 0.0, "h"),
                                                                    (40, 10.5, 25, 0.0, "h")]))
    index.append(run_tape("idm_placed_rear_end", 1, 0.5, placement=[(120, 0.0, 1, 0.0, "h"), (111, 0.0, 30, 0.0, "h"),
                                                                    (60, 10.5, 25, 0.0, "h"), (20, 0.0, 25, 0.0, "h")]))
    index.append(run_tape("idm_placed_x_neg", 2, 1.2, placement=[(-9, 0.0, 2, 0.0, "h"), (80, 0.0, 25, 0.0, "h"),
                                                                 (30, 10.5, 26, 0.0, "h"), (160, 0.0, 27, 0.0, "h")]))
    with open(os.path.join(OUT, "idm_index.json"), "w") as f:
        json.dump(index, f, indent=1)
    gen_reset()


if __name__ == "__main__":
    main()
