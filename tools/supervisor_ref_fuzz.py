#!/usr/bin/env python3
"""The reference's safety_supervisor against its CPU twin (oracle/mm_oracle.c mm_supervise, math mode 0) on the same states
with the same recorded draws.  Runs in the build container only, like tools/gen_golden_priority.py: the reference is imported
under tools/refshim.

    python tools/supervisor_ref_fuzz.py [--states 20000] [--procs 8] [--seed 1]      # the fuzz -> profiles/supervisor_twin/ref_fuzz.json
    python tools/supervisor_ref_fuzz.py --record-placed                               # tests/golden/sup_placed_*.npz + index

States: natural episodes (traffic densities 1-3, CAV-only and mixed, HEADWAY_TIME 0.5 and 1.2, action distributions skewed
to FASTER and to lane changes, every step of every episode) and the placed states of tests/supervisor_twin_util.placed_scenes
under several lookahead horizons, built to reach every census entry.  Per state the reference call is wrapped: np.random.rand
records the draws, PriorityQueue.put the priority numbers, copy.deepcopy hands out env_copy.  The twin gets the state, the
joint action and the draws, and must return the same action, consume the same number of draws, take the vehicles in the same
order, and end with the same lookahead copy: every vehicle's trajectory points (a crashed HDV's aliased points included) and
live state.  Both sides evaluate libm in the same operation order, so a difference above TOL = 1e-9 is a finding, and a
flipped decision is one whatever its size.  Exit status 1 on any finding.
"""
import argparse
import copy
import json
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (puts the reference and the shims on sys.path)
import gen_golden_priority as gp  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import highway_env.envs.common.abstract as habs  # noqa: E402
import highway_env.vehicle.safety.central_layer as hcl  # noqa: E402
from highway_env.vehicle.controller import MDPVehicle  # noqa: E402

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import supervisor_twin_util as U  # noqa: E402

TOL = U.TOL
PROFILE = os.path.join(REPO, "profiles", "supervisor_twin", "ref_fuzz.json")
HORIZONS = ((1, 15), (6, 15), (8, 15), (6, 5), (10, 15))  # (n_step, simulation_frequency) at policy_frequency 5
SKEWS = {"fast": [0.15, 0.15, 0.1, 0.5, 0.1], "lc": [0.3, 0.1, 0.2, 0.3, 0.1], "faster": [0.05, 0.1, 0.05, 0.75, 0.05]}


def reference_call(env, actions):
    """safety_supervisor(env, actions) with its draws, its priority numbers and its env_copy captured."""
    draws, keys, copies = [], [], []
    rand, put, deep = np.random.rand, hcl.PriorityQueue.put, copy.deepcopy

    def rec_rand(*a):
        r = rand(*a)
        draws.append(float(r))
        return r

    def rec_put(q, item, *a, **k):
        keys.append((float(item[0]), int(item[1][2])))
        return put(q, item, *a, **k)

    def rec_deep(x, *a, **k):
        y = deep(x, *a, **k)
        if x is env and not copies:
            copies.append(y)
        return y
    np.random.rand, hcl.PriorityQueue.put, copy.deepcopy = rec_rand, rec_put, rec_deep
    try:
        out = gp._orig_sup(env, actions, True)
    finally:
        np.random.rand, hcl.PriorityQueue.put, copy.deepcopy = rand, put, deep
    return tuple(int(a) for a in out), draws, keys, copies[0]


def snapshot(env):
    """The state the supervisor sees as the arrays tests/supervisor_twin_util.put_state takes (one row)."""
    vs = env.road.vehicles
    st = {"x": [v.position[0] for v in vs], "y": [v.position[1] for v in vs], "heading": [v.heading for v in vs],
          "speed": [v.speed for v in vs], "target_speed": [v.target_speed for v in vs],
          "lane": [gg.LANE_ID[tuple(v.lane_index)] for v in vs], "target_lane": [gg.LANE_ID[tuple(v.target_lane_index)] for v in vs],
          "speed_index": [int(getattr(v, "speed_index", 0)) for v in vs], "crashed": [int(bool(v.crashed)) for v in vs],
          "kind": [1 if isinstance(v, MDPVehicle) else 2 for v in vs]}
    return {k: np.asarray(v, dtype=np.float64 if k in U.F_KEYS else np.int64)[None] for k, v in st.items()}


def copy_arrays(env_copy, n_points):
    """env_copy after the call in the Trace.parse() arrangement of one env."""
    vs = env_copy.road.vehicles
    m = len(vs)
    ln = np.zeros(m, dtype=np.int64)
    live = np.zeros((m, 9))
    pts = np.zeros((m, n_points, 4))
    for k, v in enumerate(vs):
        tr = v.trajectories
        ln[k] = len(tr)
        hdv = not isinstance(v, MDPVehicle)
        live[k] = [v.position[0], v.position[1], v.heading, v.speed, v.target_speed, gg.LANE_ID[tuple(v.target_lane_index)],
                   float(bool(v.crashed)), float(v.action["steering"]) if hdv and tr else 0.0,
                   float(v.action["acceleration"]) if hdv and tr else 0.0]
        for t, p in enumerate(tr):
            aliased = p[0] is v.position
            pts[k, t] = [np.nan if aliased else p[0][0], np.nan if aliased else p[0][1], p[1], p[2]]
    return ln, live, pts


class Batch(object):
    """States of one shape (m vehicles, one horizon, one HEADWAY_TIME) compared with the twin in one call."""

    def __init__(self, m, n_step, sim_freq, headway_time):
        self.m, self.n_step, self.sim_freq, self.ht = m, n_step, sim_freq, headway_time
        self.n_points = (sim_freq // 5) * n_step
        self.rows = []

    def add(self, env, actions, tag):
        st = snapshot(env)
        new, draws, keys, env_copy = reference_call(env, tuple(actions))
        self.rows.append(dict(st=st, actions=list(actions), new=new, draws=draws, order=[ix for _, ix in sorted(keys)],
                              keys=[k for k, _ in sorted(keys, key=lambda r: r[1])], copy=copy_arrays(env_copy, self.n_points), tag=tag))
        return new

    def compare(self, res):
        if not self.rows:
            return
        E, m = len(self.rows), self.m
        oe = U.oracle()
        oe.set_math_mode(0)
        cfg = {"safety_guarantee": "priority", "HEADWAY_TIME": self.ht, "n_step": self.n_step, "simulation_frequency": self.sim_freq}
        env = oe.OracleEnv(E, m, env_id="merge-multi-agent-v0", config=cfg, obs_f64=True, n_hdv=1 if m > 1 else 0)
        U.put_state(env, U.cat_states([r["st"] for r in self.rows]))
        act = np.ones((E, m), dtype=np.int32)
        Ud = np.zeros((E, 9 * m))
        for e, r in enumerate(self.rows):
            act[e, :len(r["actions"])] = r["actions"]
            Ud[e, :len(r["draws"])] = r["draws"]
        with U.Trace(E, m, self.n_points) as tr:
            new, nd = env.supervise(torch.as_tensor(act), uniforms=Ud)
            tw = tr.parse()
        U.add_census(res["census"], U.census())
        new, nd = new.numpy(), nd.numpy()
        for e, r in enumerate(self.rows):
            n = len(r["actions"])
            res["states"] += 1
            res["by_tag"][r["tag"]] = res["by_tag"].get(r["tag"], 0) + 1
            bad = []
            if tuple(new[e, :n]) != r["new"]:
                bad.append("new_action %s vs reference %s" % (new[e, :n].tolist(), list(r["new"])))
            if int(nd[e]) != len(r["draws"]):
                bad.append("n_draws %d vs %d" % (nd[e], len(r["draws"])))
            if tw["order"][e, :n].tolist() != r["order"]:
                bad.append("order %s vs %s" % (tw["order"][e, :n].tolist(), r["order"]))
            ln, live, pts = r["copy"]
            if not np.array_equal(tw["len"][e], ln):
                bad.append("trajectory lengths %s vs %s" % (tw["len"][e].tolist(), ln.tolist()))
            else:
                has = ln > 0
                used = (np.arange(self.n_points)[None, :] < ln[:, None])[..., None] & np.ones(4, dtype=bool)
                if not np.array_equal(np.isnan(tw["points"][e])[used], np.isnan(pts)[used]):
                    bad.append("aliased points differ")
                else:
                    dev = max(float(np.nanmax(np.abs(tw["points"][e] - pts)[used], initial=0.0)),
                              float(np.abs(tw["live"][e] - live)[has].max(initial=0.0)),
                              float(np.abs(tw["key"][e, :n] - np.asarray(r["keys"])).max(initial=0.0)))
                    res["worst_deviation"] = max(res["worst_deviation"], dev)
                    if dev > TOL:
                        bad.append("trace deviation %.3g" % dev)
            if bad:
                res["findings"].append(dict(tag=r["tag"], what=bad, state={k: v[0].tolist() for k, v in r["st"].items()},
                                            actions=r["actions"], draws=r["draws"], n_step=self.n_step, simulation_frequency=self.sim_freq,
                                            headway_time=self.ht))
        self.rows = []


def make_env(n, n_hdv, ht, n_step=6, sim_freq=15):
    env = gg.make_env("merge-multi-agent-v0", "priority", n, ht, 0.0, n_hdv=n_hdv)
    env.config["n_step"] = n_step
    env.config["simulation_frequency"] = sim_freq
    env.config["action_masking"] = True
    return env


def place_scene(env, vs):
    """A placed scene of supervisor_twin_util in the reference env: creation order, then the fields a spawn cannot set."""
    gg._place_vehicles(env, [(v["x"], v["y"], v["speed"], v["heading"]) + (("h",) if v["kind"] == 2 else ()) for v in vs])
    for v, r in zip(vs, env.road.vehicles):
        r.target_speed = float(v["target_speed"])
        r.crashed = bool(v["crashed"])
        r.target_lane_index = gg.LANE_IX[v["target_lane"]]
        if v["kind"] == 1:
            r.speed_index = int(v["speed_index"])
        assert gg.LANE_ID[tuple(r.lane_index)] == v["lane"], "the oracle's closest lane differs from the reference's"


def natural(res, seed, target):
    """Natural episodes until `target` supervised states are compared."""
    rng = np.random.RandomState(seed)
    dens = {1: ((1, 3), (1, 3)), 2: ((2, 4), (2, 4)), 3: ((4, 6), (3, 5))}  # merge_env_v1.py:180-211
    done_states = 0
    while done_states < target:
        d = int(rng.randint(1, 4))
        nc, nh = int(rng.randint(dens[d][0][0], dens[d][0][1] + 1)), int(rng.randint(dens[d][1][0], dens[d][1][1] + 1))
        mixed = bool(rng.randint(2))
        n, h = (nc, nh) if mixed else (nc + nh, 0)
        ht = float(rng.choice([0.5, 1.2]))
        skew = str(rng.choice(sorted(SKEWS)))
        env = make_env(n, h, ht)
        env.seed = int(rng.randint(1 << 30))
        np.random.seed(env.seed)
        env.reset()
        b = Batch(len(env.road.vehicles), 6, 15, ht)
        tag = "natural_d%d_%s_ht%s_%s" % (d, "mixed" if mixed else "cav", ht, skew)
        habs.safety_supervisor = lambda env, actions: b.add(env, actions, tag)  # noqa: E731
        try:
            for _ in range(100):
                a = tuple(int(x) for x in rng.choice(5, n, p=SKEWS[skew]))
                _, _, d_, _ = env.step(a)
                if d_:
                    break
        finally:
            habs.safety_supervisor = gp._recording_supervisor
        done_states += len(b.rows)
        b.compare(res)


def placed(res, seed, per_family):
    for (n_step, sim_freq) in HORIZONS:
        batches = {}
        for k, (fam, vs, acts) in enumerate(U.placed_scenes(seed, per_family)):
            ht = 0.5 if k % 2 else 1.2
            n = sum(1 for v in vs if v["kind"] == 1)
            env = make_env(n, len(vs) - n, ht, n_step, sim_freq)
            env.seed = 1
            env.reset()
            place_scene(env, vs)
            if k % 4 == 3:  # action codes outside 0..4 pass through unless replaced
                acts = list(acts)
                acts[k % n] = [-1, 5, 7, 100][(k // 4) % 4]
            b = batches.setdefault((len(vs), ht), Batch(len(vs), n_step, sim_freq, ht))
            np.random.seed(seed + k)
            b.add(env, acts, "placed_%s_n%d_f%d" % (fam, n_step, sim_freq))
        for b in batches.values():
            b.compare(res)


def worker(job):
    kind, seed, amount = job
    res = dict(states=0, census={}, worst_deviation=0.0, findings=[], by_tag={})
    if kind == "natural":
        natural(res, seed, amount)
    else:
        placed(res, seed, amount)
    return res


def fuzz(args):
    per = -(-args.states // args.procs)
    jobs = [("natural", args.seed * 1000 + k, per) for k in range(args.procs)] + [("placed", 20261019 + s, 40) for s in range(args.placed_seeds)]
    with multiprocessing.Pool(args.procs) as pool:
        parts = pool.map(worker, jobs, chunksize=1)
    tot = dict(states=0, census={}, worst_deviation=0.0, findings=[], by_tag={})
    for r in parts:
        tot["states"] += r["states"]
        U.add_census(tot["census"], r["census"])
        U.add_census(tot["by_tag"], r["by_tag"])
        tot["worst_deviation"] = max(tot["worst_deviation"], r["worst_deviation"])
        tot["findings"] += r["findings"]
    natural_states = sum(v for k, v in tot["by_tag"].items() if k.startswith("natural"))
    out = dict(tool="tools/supervisor_ref_fuzz.py", math_mode=0, tolerance=TOL, states=tot["states"], natural_states=natural_states,
               placed_states=tot["states"] - natural_states, decision_differences=len(tot["findings"]),
               worst_trace_deviation=tot["worst_deviation"], census=tot["census"],
               census_missing=[k for k in U.CENSUS_REQUIRED if tot["census"].get(k, 0) < U.CENSUS_MIN],
               states_by_family={k: tot["by_tag"][k] for k in sorted(tot["by_tag"])}, findings=tot["findings"][:20],
               compared="new_action, n_draws, priority order and numbers, every vehicle's final trajectories and live state in env_copy")
    os.makedirs(os.path.dirname(PROFILE), exist_ok=True)
    with open(PROFILE, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("states", "natural_states", "placed_states", "decision_differences", "worst_trace_deviation",
                                          "census_missing")}))
    return 1 if tot["findings"] else 0


def record_placed(args):
    """tests/golden/sup_placed_*.npz: one short reference episode per family of placed states, in the prio_* field layout
    (tools/gen_golden_priority.run_tape), plus sup_placed_index.json with the twin's census of each tape."""
    index = []
    plans = [(fam, 6, 15) for fam in U.FAMILIES] + [("crashed_hdv", 1, 15), ("four_slots_ramp", 8, 15), ("obstacle", 6, 5), ("speeds", 10, 15)]
    scenes = U.placed_scenes(20261019, 4)
    for k, (fam, n_step, sim_freq) in enumerate(plans):
        _, vs, acts = [s for s in scenes if s[0] == fam][k % 4]
        n, ht = sum(1 for v in vs if v["kind"] == 1), (0.5 if k % 2 else 1.2)
        env = make_env(n, len(vs) - n, ht, n_step, sim_freq)
        env.seed = 1
        env.reset()
        place_scene(env, vs)
        habs.safety_supervisor = gp._recording_supervisor
        gp._REC = rec = []
        rng = np.random.RandomState(k)
        rewards, dones, obs, masks = [], [], [], []
        np.random.seed(100 + k)
        for t in range(8):
            a = tuple(acts) if t == 0 else tuple(int(x) for x in rng.choice(5, n, p=SKEWS["fast"]))
            o, r, d, info = env.step(a)
            rewards.append(r), dones.append(d), masks.append(np.asarray(info["action_mask"]))
            obs.append(np.asarray(o, dtype=np.float64).reshape(n, -1))
            if d:
                break
        gp._REC = None
        T, m = len(rec), len(env.road.vehicles)
        Ud = np.full((T, 9 * m), np.nan)
        for t, r in enumerate(rec):
            Ud[t, :len(r["draws"])] = r["draws"]
        z = dict(pre_f=np.array([r["f"] for r in rec], dtype=np.float64), pre_i=np.array([r["i"] for r in rec], dtype=np.int32),
                 actions=np.array([r["actions"] for r in rec], dtype=np.int32), new_actions=np.array([r["new"] for r in rec], dtype=np.int32),
                 uniforms=Ud, n_draws=np.array([len(r["draws"]) for r in rec], dtype=np.int32),
                 order=np.array([r["order"] for r in rec], dtype=np.int32), sub_f=np.array([r["sf"] for r in rec], dtype=np.float64),
                 sub_i=np.array([r["si"] for r in rec], dtype=np.int32), obs=np.array(obs), action_mask=np.array(masks, dtype=np.uint8),
                 rewards=np.array(rewards), dones=np.array(dones, dtype=np.uint8))
        name = "sup_placed_%s_n%d_f%d" % (fam, n_step, sim_freq)
        meta = dict(env_id="merge-multi-agent-v0", shield="priority", n=n, n_hdv=m - n, headway_time=ht, seed=1, n_step=n_step,
                    simulation_frequency=sim_freq, n_merge=int(env.n_merge), family=fam, compat=False)
        np.savez_compressed(os.path.join(gg.OUT, name + ".npz"), meta=json.dumps(meta), **z)
        # the twin's census of the tape (teacher-forced, math mode 0)
        oe = U.oracle()
        oe.set_math_mode(0)
        tenv = oe.OracleEnv(T, m, env_id="merge-multi-agent-v0", config=U.tape_config(meta), obs_f64=True, n_hdv=min(m - n, 1))
        U.put_state(tenv, U.tape_state(z), steps=np.arange(T), n_merge=meta["n_merge"])
        act = np.ones((T, m), dtype=np.int32)
        act[:, :n] = z["actions"]
        new, _ = tenv.supervise(torch.as_tensor(act), uniforms=np.nan_to_num(Ud))
        assert np.array_equal(new.numpy()[:, :n], z["new_actions"]), name
        cen = {k_: v for k_, v in U.census().items() if v}
        index.append(dict(name=name, steps=T, replaced=int((z["actions"] != z["new_actions"]).sum()), family=fam, census=cen))
        print("%-40s T=%d replaced=%d" % (name, T, index[-1]["replaced"]))
    with open(os.path.join(gg.OUT, "sup_placed_index.json"), "w") as f:
        json.dump(index, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=20000, help="natural supervised states to compare (placed ones come on top)")
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--placed-seeds", type=int, default=2)
    ap.add_argument("--record-placed", action="store_true")
    args = ap.parse_args()
    if args.record_placed:
        return record_placed(args)
    return fuzz(args)


if __name__ == "__main__":
    sys.exit(main())
