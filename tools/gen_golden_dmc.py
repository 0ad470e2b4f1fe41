#!/usr/bin/env python3
"""Golden tapes of the reference's "dmc" safety supervisor (runs in the build container only).

Imports the reference under tools/refshim as tools/gen_golden_priority.py does, wraps safety_layer_dmc
(decentralised_dmc.py:70-193) and records, per call, the state it sees, the joint action, its np.random.rand() values, the
action it returns and, per vehicle, the stages in between (the trace of include/mm_supervisor.h, mm_supervise_dmc).  The
outputs are DATA only: tests/golden/dmc_*.npz and tests/golden/dmc_index.json.

    python tools/gen_golden_dmc.py

Per tape (n controlled vehicles, m vehicles on the road, T kept states): meta (json); sub_f [T][m][11] / sub_i [T][m][9]
(columns of gen_golden._veh_snapshot); actions / new_actions [T][n]; uniforms [T][2m] (NaN-padded); n_draws [T]; order
[T][n]; trace [T][m][20]; hit [T][n] (what the vehicle collided with: -1 nothing, 0..3 the neighbour list index of
[v_fl, v_rr, v_fr, v_rl], 4 the obstacle); hdv_front [T][m] (front vehicle generate_actions saw: -1 none, -2 the obstacle,
else its slot; -3: not an HDV); step [T] (index of the state in its episode); obs [T][n][25], rewards, dones, action_mask
[T][n][5] of the env step that followed.

Knife edges: every state is run through the reference twice more with all positions and speeds shifted by +-1e-9 (same
draws); a state whose new_actions, crash_t or neighbour slots change is dropped.  At most 2 % may be dropped per tape and
overall: asserted here.  dmc_index.json holds the kept / dropped counts and the census of tests/dmc_util.census.
"""
import copy
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "tests")]
import gen_golden as gg  # noqa: E402  (puts the reference and the shims on sys.path)
import numpy as np  # noqa: E402
import highway_env.envs.common.abstract as habs  # noqa: E402
import highway_env.envs.common.idm_controller as hidm  # noqa: E402
import highway_env.vehicle.safety.decentralised_dmc as hdmc  # noqa: E402
from highway_env.road.objects import Obstacle  # noqa: E402
import dmc_util as D  # noqa: E402  (numpy-only at import: the census and the trace layout)

OUT = gg.OUT
EPS = 1e-9
MAX_DROP = 0.02
_orig_dmc = hdmc.safety_layer_dmc
_REC = None


def _slot(vehicles, v):
    for k, u in enumerate(vehicles):
        if u is v:
            return k
    return -2 if isinstance(v, Obstacle) else -1


def traced_dmc(env, actions, draws=None):
    """safety_layer_dmc with every stage recorded.  draws: replay these np.random.rand() values instead of drawing."""
    m = len(env.road.vehicles)
    n = len(env.controlled_vehicles)
    tr = np.full((m, D.TRACE), np.nan)
    tr[:, D.T_POS] = -1
    tr[:, D.T_CRASH] = -1
    tr[:, D.T_FL:D.T_RL + 1] = -1
    tr[:, D.T_MASK] = 0
    hit = np.full(n, -1, dtype=np.int32)
    front = np.full(m, -3, dtype=np.int32)
    used, keys, state = [], [], dict(pos=0, cur=None, copy=None)
    rand, put = np.random.rand, hdmc.PriorityQueue.put
    ev, gen = hdmc._evaluate_vehicle_action, hdmc.generate_actions
    room, coll = habs.AbstractEnv.check_safety_room, habs.AbstractEnv.check_collision
    it = iter(draws) if draws is not None else None

    def rec_rand(*a):
        r = next(it) if it is not None else rand(*a)
        used.append(float(r))
        return r

    def rec_put(q, item, *a, **k):
        keys.append((item[0], item[1][2]))
        return put(q, item, *a, **k)

    def rec_gen(vehicle, env_copy):
        s = _slot(env_copy.road.vehicles, vehicle)
        f, _ = hidm.neighbour_vehicles(vehicle, env_copy)
        front[s] = -1 if f is None else _slot(env_copy.road.vehicles, f)
        a = gen(vehicle, env_copy)
        tr[s, D.T_HS], tr[s, D.T_HA] = float(a["steering"]), float(a["acceleration"])  # (clip_actions rewrites the dict later)
        return a

    def rec_room(self, vehicle, action, surrounding, env_copy, time_steps):
        r = room(self, vehicle, action, surrounding, env_copy, time_steps)
        s = state["cur"]
        tr[s, D.T_ROOM + action] = r if time_steps == 0 else tr[s, D.T_ROOM + action] + r
        return r

    def rec_coll(self, vehicle, other, other_trajectories):
        before = vehicle.crashed
        coll(self, vehicle, other, other_trajectories)
        if state["cur"] is not None and not before and vehicle.crashed:
            hit[state["cur"]] = 4 if isinstance(other, Obstacle) else [k for k, u in enumerate(state["nb"]) if u is other][0]

    def rec_ev(vehicle, original_vehicle, available_actions, env_copy, n_points, neighbours):
        vs = env_copy.road.vehicles
        if state["copy"] is None:  # before step 2 touches anything: the end of every propagation
            state["copy"] = True
            for k, u in enumerate(vs):
                tr[k, D.T_EX:D.T_EV + 1] = [u.position[0], u.position[1], u.heading, u.speed]
                tr[k, D.T_STAND] = u.position[0]
        s = _slot(vs, vehicle)
        state["cur"], state["nb"] = s, neighbours
        tr[s, D.T_POS] = state["pos"]
        state["pos"] += 1
        tr[s, D.T_FL:D.T_RL + 1] = [-1 if u is None else _slot(vs, u) for u in neighbours]
        tr[s, D.T_MASK] = sum(1 << int(a) for a in available_actions)
        sel = ev(vehicle, original_vehicle, available_actions, env_copy, n_points, neighbours)
        if sel is not None:  # the crash-time point IS the vehicle's position object (decentralised_dmc.py:35)
            tr[s, D.T_CRASH] = [t for t in range(n_points) if vehicle.position is vehicle.trajectories[t][0]][0]
        tr[s, D.T_STAND] = vehicle.position[0]
        state["cur"] = None
        return sel

    np.random.rand, hdmc.PriorityQueue.put = rec_rand, rec_put
    hdmc._evaluate_vehicle_action, hdmc.generate_actions = rec_ev, rec_gen
    habs.AbstractEnv.check_safety_room, habs.AbstractEnv.check_collision = rec_room, rec_coll
    try:
        out = _orig_dmc(env, actions)
    finally:
        np.random.rand, hdmc.PriorityQueue.put = rand, put
        hdmc._evaluate_vehicle_action, hdmc.generate_actions = ev, gen
        habs.AbstractEnv.check_safety_room, habs.AbstractEnv.check_collision = room, coll
    for k, ix in keys:
        tr[ix, D.T_KEY] = k
    return dict(new=[int(a) for a in out], draws=used, order=[ix for _, ix in sorted(keys)], trace=tr, hit=hit, front=front)


def _shifted(env, eps):
    e2 = copy.deepcopy(env)
    for v in e2.road.vehicles:
        v.position = v.position + eps
        v.speed = v.speed + eps
    return e2


def _recording_dmc(env, actions):
    snap = [gg._veh_snapshot(v) for v in env.road.vehicles]
    r = traced_dmc(env, actions)
    if _REC is not None:
        stable = True
        for eps in (EPS, -EPS):
            try:
                q = traced_dmc(_shifted(env, eps), actions, draws=r["draws"])
            except Exception:  # the shifted state left the reference's domain
                stable = False
                break
            if q["new"] != r["new"] or not np.array_equal(q["trace"][:, D.T_CRASH:D.T_RL + 1], r["trace"][:, D.T_CRASH:D.T_RL + 1]):
                stable = False
                break
        r.update(sf=[s[0] for s in snap], si=[s[1] for s in snap], actions=[int(a) for a in actions], stable=stable)
        _REC.append(r)
    return tuple(r["new"])


habs.safety_layer_dmc = _recording_dmc


def make_env(n, n_hdv, ht, n_step=6, sim_freq=15, policy_freq=5):
    env = gg.make_env("merge-multi-agent-v0", "dmc", n, ht, 0.0, n_hdv=n_hdv)
    env.config["n_step"] = n_step
    env.config["simulation_frequency"] = sim_freq
    env.config["policy_frequency"] = policy_freq
    env.config["action_masking"] = True
    return env


def save_tape(name, rec, results, meta):
    """rec: the recorded calls, results: (obs, reward, done, mask, step) of the env step after each; drops the knife edges."""
    keep = [k for k, r in enumerate(rec) if r["stable"]][:4096]
    dropped = len(rec) - sum(1 for r in rec if r["stable"])
    assert dropped <= MAX_DROP * len(rec), "%s: %d of %d states are knife edges" % (name, dropped, len(rec))
    m, n = len(rec[0]["sf"]), len(rec[0]["actions"])
    U = np.full((len(keep), 2 * m), np.nan)
    for j, k in enumerate(keep):
        U[j, :len(rec[k]["draws"])] = rec[k]["draws"]
    col = lambda key, dt: np.array([rec[k][key] for k in keep], dtype=dt)  # noqa: E731
    z = dict(sub_f=col("sf", np.float64), sub_i=col("si", np.int32), actions=col("actions", np.int32), new_actions=col("new", np.int32),
             uniforms=U, n_draws=np.array([len(rec[k]["draws"]) for k in keep], dtype=np.int32), order=col("order", np.int32),
             trace=col("trace", np.float64), hit=col("hit", np.int32), hdv_front=col("front", np.int32),
             step=np.array([results[k][4] for k in keep], dtype=np.int32),
             obs=np.array([results[k][0] for k in keep]), rewards=np.array([results[k][1] for k in keep], dtype=np.float64),
             dones=np.array([results[k][2] for k in keep], dtype=np.uint8), action_mask=np.array([results[k][3] for k in keep], dtype=np.uint8))
    meta = dict(meta, env_id="merge-multi-agent-v0", shield="dmc", n=n, n_hdv=m - n)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), meta=json.dumps(meta), **z)
    repl = int((z["actions"] != z["new_actions"]).sum())
    print("%-36s kept=%4d dropped=%d replaced=%d" % (name, len(keep), dropped, repl))
    return dict(name=name, kept=len(keep), dropped=dropped, replaced=repl, n=n, n_hdv=m - n, census=D.census(z, meta))


def run_natural(name, n, n_hdv, ht, seed, p, episodes=3, n_step=6, sim_freq=15, compat=False, steps=60, policy_freq=5):
    """Natural episodes (the first one from `seed`), stitched into one tape; step restarts at 0 with every episode."""
    global _REC
    rec, results, n_merge = [], [], None
    for ep in range(episodes):
        env = make_env(n, n_hdv, ht, n_step, sim_freq, policy_freq)
        env.seed = seed + ep
        env.reset()
        if n_merge is None:
            n_merge = int(env.n_merge)
        if int(env.n_merge) != n_merge:  # (N_MERGE is one number per tape)
            continue
        rng = np.random.RandomState(seed + 1000 + ep)
        _REC = []
        for t in range(steps):
            a = tuple(int(x) for x in (np.random.choice(5, n, p=p) if compat else rng.choice(5, n, p=p)))
            o, r, d, info = env.step(a)
            results.append((np.asarray(o, dtype=np.float64).reshape(n, -1), r, d, np.asarray(info["action_mask"]), t))
            if d:
                break
        rec += _REC
        _REC = None
    meta = dict(headway_time=ht, seed=seed, n_step=n_step, simulation_frequency=sim_freq, policy_frequency=policy_freq, p=list(p),
                n_merge=n_merge, compat=bool(compat), natural=True, episodes=episodes)
    return save_tape(name, rec, results, meta)


def run_placed(name, fam, scenes, ht, n_step=6, sim_freq=15):
    """One reference call (and the env step after it) per placed scene of a family with the same vehicle counts."""
    global _REC
    import supervisor_ref_fuzz as rf
    habs.safety_layer_dmc = _recording_dmc  # (supervisor_ref_fuzz's imports patch the priority hook only)
    rec, results = [], []
    for k, (_, vs, acts) in enumerate(scenes):
        n = sum(1 for v in vs if v["kind"] == 1)
        env = make_env(n, len(vs) - n, ht, n_step, sim_freq)
        env.seed = 1
        env.reset()
        rf.place_scene(env, vs)
        np.random.seed(500 + k)
        _REC = []
        try:
            o, r, d, info = env.step(tuple(acts))
        except Exception as ex:  # a state on which the reference itself raises is outside the domain: not recorded
            print("  %s scene %d: reference raised %s" % (fam, k, type(ex).__name__))
            _REC = None
            continue
        results.append((np.asarray(o, dtype=np.float64).reshape(n, -1), r, d, np.asarray(info["action_mask"]), 0))
        rec += _REC
        _REC = None
    meta = dict(headway_time=ht, seed=1, n_step=n_step, simulation_frequency=sim_freq, policy_frequency=5, n_merge=0, compat=False, natural=False, family=fam)
    return save_tape(name, rec, results, meta)


FAST = [0.15, 0.15, 0.1, 0.5, 0.1]   # towards FASTER (and lane changes) so that lookaheads crash
LC = [0.3, 0.1, 0.2, 0.3, 0.1]
FASTER = [0.05, 0.1, 0.05, 0.75, 0.05]


def main():
    import supervisor_twin_util as U
    index = []
    plans = [(4, 0, 1.2, LC, "lc"), (6, 0, 0.5, FAST, "fast"), (8, 0, 0.5, FASTER, "faster"), (8, 0, 1.2, LC, "lc"),
             (3, 3, 1.2, FAST, "fast"), (4, 4, 0.5, FASTER, "faster"), (4, 4, 1.2, LC, "lc"), (6, 5, 0.5, FASTER, "faster"),
             (6, 5, 1.2, FAST, "fast")]
    seed = 0
    for (n, h, ht, p, tag) in plans:
        seed += 25
        mix = "%dc%dh" % (n, h) if h else "N%d" % n
        index.append(run_natural("dmc_v0_%s_ht%s_%s_s%d" % (mix, str(ht).replace(".", ""), tag, seed), n, h, ht, seed, p, episodes=4))
    index.append(run_natural("dmc_v0_4c4h_ht05_nstep1_s300", 4, 4, 0.5, 300, FASTER, episodes=2, n_step=1))
    index.append(run_natural("dmc_v0_N8_ht12_nstep2_s325", 8, 0, 1.2, 325, FASTER, episodes=2, n_step=2))
    # simulation_frequency 25 at policy_frequency 10: 2 sub-steps per policy step of 1 / 25 s (the env steps at most 3)
    index.append(run_natural("dmc_v0_6c5h_ht05_f25_s350", 6, 5, 0.5, 350, FASTER, episodes=2, sim_freq=25, policy_freq=10, steps=120))
    scenes = U.placed_scenes(20261020, 24)
    for k, fam in enumerate(U.FAMILIES):
        by_shape = {}
        for s in scenes:
            if s[0] == fam:
                by_shape.setdefault((len(s[2]), len(s[1])), []).append(s)
        for (n, m), ss in sorted(by_shape.items()):
            index.append(run_placed("dmc_placed_%s_%dc%dh" % (fam, n, m - n), fam, ss, 0.5 if k % 2 else 1.2))
    index.append(run_placed("dmc_placed_left_only_1c1h", "left_only", D.left_only_scenes(20261021, 64), 0.5))
    index.append(run_placed("dmc_placed_faster_wins_1c1h_nstep1", "faster_wins", D.faster_wins_scenes(20261022, 40), 0.5, n_step=1))
    index.append(run_natural("dmc_compat_4c4h_s7", 4, 4, 0.5, 7, FAST, episodes=1, compat=True, steps=25))
    total = D.total_census(r["census"] for r in index)
    kept, dropped = sum(r["kept"] for r in index), sum(r["dropped"] for r in index)
    assert dropped <= MAX_DROP * (kept + dropped), "knife edges: %d of %d" % (dropped, kept + dropped)
    with open(os.path.join(OUT, "dmc_index.json"), "w") as f:
        json.dump(dict(kept=kept, dropped=dropped, census=total, tapes=index), f, indent=1)
    print("kept %d dropped %d replaced %d" % (kept, dropped, sum(r["replaced"] for r in index)))
    print(json.dumps(total, indent=1))


if __name__ == "__main__":
    main()
