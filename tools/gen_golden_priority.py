#!/usr/bin/env python3
"""Golden tapes of the reference's "priority" safety supervisor (runs in the build container only).

Imports the reference under tools/refshim exactly as tools/gen_golden.py does and records, for every step of a v0
CAV-only or mixed-traffic episode, the state the supervisor sees, the joint action, the np.random.rand() values it drew (recorded by
wrapping np.random.rand while it runs) and the action it returns.  The outputs are DATA only (tests/golden/prio_*.npz,
tests/golden/prio_index.json); prefix prio_ keeps them out of golden_util.episode_files.

    python tools/gen_golden_priority.py

Per tape (n controlled vehicles, m vehicles on the road): meta (json); sub_f [T][m][11] / sub_i [T][m][9] the state
every vehicle has when step t starts (columns of gen_golden._veh_snapshot); pre_f / pre_i the supervisor's view of it
(x, y, heading, speed, target_speed / lane, target_lane, speed_index, crashed, [m]); actions / new_actions [T][n];
uniforms [T][9m] (NaN-padded); n_draws [T]; order [T][n] (controlled indices, smallest key first); obs [T][n][25],
rewards, dones, action_mask [T][n][5] of the step.  prio_compat_* tapes run on the natural global stream
(np.random.seed(s); reset; step ...) with no injected draws, for the MergeEnvCompat adapter.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (puts the reference and the shims on sys.path)
import numpy as np  # noqa: E402
import highway_env.envs.common.abstract as habs  # noqa: E402
import highway_env.vehicle.safety.central_layer as hcl  # noqa: E402

OUT = gg.OUT
_orig_sup = hcl.safety_supervisor
_REC = None


def _recording_supervisor(env, actions, is_priority=True):
    """safety_supervisor with its inputs, its draws and its result recorded."""
    vs = env.road.vehicles
    snap = [gg._veh_snapshot(v) for v in vs]
    f = [[v.position[0], v.position[1], v.heading, v.speed, v.target_speed] for v in vs]
    i = [[gg.LANE_ID[tuple(v.lane_index)], gg.LANE_ID[tuple(v.target_lane_index)], int(getattr(v, "speed_index", 0)),
          int(bool(v.crashed))] for v in vs]
    draws = []
    rand = np.random.rand

    def rec_rand(*a):
        r = rand(*a)
        draws.append(float(r))
        return r
    order = []
    put = hcl.PriorityQueue.put

    def rec_put(q, item, *a, **k):
        order.append((item[0], item[1][2]))
        return put(q, item, *a, **k)
    np.random.rand = rec_rand
    hcl.PriorityQueue.put = rec_put
    try:
        out = _orig_sup(env, actions, is_priority)
    finally:
        np.random.rand = rand
        hcl.PriorityQueue.put = put
    if _REC is not None:
        _REC.append(dict(f=f, i=i, sf=[r[0] for r in snap], si=[r[1] for r in snap], actions=list(actions), new=list(out), draws=draws,
                         order=[ix for _, ix in sorted(order)]))
    return out


habs.safety_supervisor = _recording_supervisor


def run_tape(name, n, headway_time, seed, p, steps=40, placement=None, n_hdv=0, compat=False):
    global _REC
    env = gg.make_env("merge-multi-agent-v0", "priority", n, headway_time, 0.0, n_hdv=n_hdv)
    env.config["n_step"] = 6
    env.config["action_masking"] = True
    env.seed = seed
    env.reset()
    if placement is not None:
        gg._place_vehicles(env, placement)
        n = len(env.controlled_vehicles)
    init = [[v.position[0], v.position[1], v.heading, v.speed] for v in env.controlled_vehicles]
    rng = np.random.RandomState(seed + 1000)
    _REC = []
    rewards, dones, obs, masks = [], [], [], []
    for t in range(steps):
        # compat tapes: the policy's draws come from the global stream too, as MAPPO's np.random.choice does
        a = tuple(int(x) for x in (np.random.choice(5, n, p=p) if compat else rng.choice(5, n, p=p)))
        o, r, d, info = env.step(a)
        rewards.append(r)
        dones.append(d)
        obs.append(np.asarray(o, dtype=np.float64).reshape(n, -1))
        masks.append(np.asarray(info["action_mask"]))
        if d:
            break
    rec, _REC = _REC, None
    T = len(rec)
    m = len(env.road.vehicles)
    U = np.full((T, 9 * m), np.nan)
    for t, r in enumerate(rec):
        U[t, :len(r["draws"])] = r["draws"]
    z = dict(
        pre_f=np.array([r["f"] for r in rec], dtype=np.float64), pre_i=np.array([r["i"] for r in rec], dtype=np.int32),
        actions=np.array([r["actions"] for r in rec], dtype=np.int32),
        new_actions=np.array([r["new"] for r in rec], dtype=np.int32), uniforms=U,
        n_draws=np.array([len(r["draws"]) for r in rec], dtype=np.int32),
        order=np.array([r["order"] for r in rec], dtype=np.int32),
        sub_f=np.array([r["sf"] for r in rec], dtype=np.float64), sub_i=np.array([r["si"] for r in rec], dtype=np.int32),
        obs=np.array(obs), action_mask=np.array(masks, dtype=np.uint8),
        init_f=np.array(init, dtype=np.float64), rewards=np.array(rewards), dones=np.array(dones, dtype=np.uint8))
    meta = dict(env_id="merge-multi-agent-v0", shield="priority", n=n, n_hdv=n_hdv, headway_time=headway_time, seed=seed,
                n_step=6, p=list(p), n_merge=int(env.n_merge), compat=bool(compat))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), meta=json.dumps(meta), **z)
    repl = int((z["actions"] != z["new_actions"]).sum())
    lc = int(((z["actions"] != z["new_actions"]) & ((z["new_actions"] == 0) | (z["new_actions"] == 2))).sum())
    print("%-34s T=%3d replaced=%d to-lane-change=%d" % (name, T, repl, lc))
    return dict(name=name, steps=T, replaced=repl, to_lane_change=lc, n_hdv=n_hdv)


FAST = [0.15, 0.15, 0.1, 0.5, 0.1]   # towards FASTER (and lane changes) so that lookaheads crash
LC = [0.3, 0.1, 0.2, 0.3, 0.1]


def main():
    index = []
    plans = [(4, 0, 1.2, LC, "lc"), (8, 0, 0.5, FAST, "fast"), (8, 0, 1.2, FAST, "fast"), (8, 0, 0.5, LC, "lc"),
             (6, 0, 1.2, FAST, "fast"), (3, 3, 1.2, FAST, "fast"), (4, 4, 0.5, FAST, "fast"), (4, 4, 1.2, LC, "lc"),
             (6, 5, 0.5, FAST, "fast"), (6, 5, 1.2, LC, "lc"), (6, 5, 0.5, LC, "lc"), (4, 4, 0.5, LC, "lc"),
             (8, 0, 0.5, FAST, "fast"), (8, 0, 1.2, FAST, "fast"), (6, 5, 0.5, FAST, "fast"), (6, 5, 0.5, FAST, "fast"),
             (6, 5, 1.2, FAST, "fast"), (6, 5, 0.5, FAST, "fast"), (8, 0, 0.5, FAST, "fast"), (4, 4, 0.5, FAST, "fast")]
    seed = 0
    for (n, h, ht, p, tag) in plans:
        for _ in range(12):  # reseed until the tape replaces at least one action
            seed += 25
            mix = "%dc%dh" % (n, h) if h else "N%d" % n
            r = run_tape("prio_v0_%s_ht%s_%s_s%d" % (mix, str(ht).replace(".", ""), tag, seed), n, ht, seed, p, n_hdv=h)
            if r["replaced"] > 0:
                index.append(r)
                break
            os.remove(os.path.join(OUT, r["name"] + ".npz"))
    # the adapter's tape: the natural global stream, mixed traffic
    r = run_tape("prio_compat_4c4h_s7", 4, 0.5, 7, FAST, n_hdv=4, compat=True, steps=25)
    index.append(r)
    with open(os.path.join(OUT, "prio_index.json"), "w") as f:
        json.dump(index, f, indent=1)
    print("replaced in total:", sum(r["replaced"] for r in index))


if __name__ == "__main__":
    main()
