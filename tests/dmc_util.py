"""Helpers of the "dmc" supervisor tests: the trace layout of mm_supervise_dmc (include/mm_supervisor.h), the census of a
dmc_* tape computed from its recorded fields (tools/gen_golden_dmc.py imports it, so the tool and the tests count alike),
and the teacher-forcing plumbing of the GPU tests.  numpy only at import; torch and the package are imported on use."""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-9
CENSUS_MIN = 20
MAX_DROP = 0.02

# trace fields per slot
TRACE = 20
T_POS, T_KEY, T_CRASH, T_FL, T_RR, T_FR, T_RL, T_MASK, T_ROOM = 0, 1, 2, 3, 4, 5, 6, 7, 8
T_EX, T_EY, T_EH, T_EV, T_HS, T_HA, T_STAND = 13, 14, 15, 16, 17, 18, 19
TRACE_INT = (T_POS, T_CRASH, T_FL, T_RR, T_FR, T_RL, T_MASK)
TRACE_FLOAT = tuple(k for k in range(TRACE) if k not in TRACE_INT)

# columns of sub_f / sub_i (tools/gen_golden._veh_snapshot)
SF = {"x": 0, "y": 1, "heading": 2, "speed": 3, "target_speed": 4, "act_steer": 5, "act_acc": 6, "timer": 10}
SI = {"lane": 0, "target_lane": 1, "speed_index": 2, "crashed": 3, "kind": 8}
AB0, BC0, BC1, CD0, JK0, KB0 = 0, 1, 2, 3, 4, 5
LANE_END = {AB0: 320.0, BC0: 420.0, BC1: 420.0, CD0: 1420.0, JK0: 220.0, KB0: 320.0}

CENSUS_REQUIRED = (
    "key_ramp", "key_speed_le0", "order_differs",
    "case_main_bc0", "case_main_ab0_ramp", "case_main_none", "case_ramp_bc1", "case_ramp_kb0", "case_ramp_none",
    "follow_road_cav", "follow_road_hdv", "lane_change_other_lane", "lane_change_same_lane",
    "hdv_front_vehicle", "hdv_front_none", "hdv_front_obstacle", "hdv_crashed_at_start", "max_speed_clip",
    "hit_fl", "hit_rr", "hit_fr", "hit_rl", "hit_obstacle",
    "replaced_by_0", "replaced_by_1", "replaced_by_3", "replaced_by_4",
    "room_tie", "crashed_standing_neighbour", "live_crashed_ego", "no_crash",
)


def census(z, meta):
    """How often the kept states of a tape reach each branch, from its recorded fields alone."""
    c = {k: 0 for k in CENSUS_REQUIRED}
    T, n = z["actions"].shape
    for t in range(T):
        sf, si, tr = z["sub_f"][t], z["sub_i"][t], z["trace"][t]
        m = sf.shape[0]
        c["order_differs"] += int(list(z["order"][t]) != list(range(n)))
        c["max_speed_clip"] += int((np.abs(sf[:, SF["speed"]]) > 40).any())
        for s in range(m):
            lane, x = int(si[s, SI["lane"]]), sf[s, SF["x"]]
            tl_end = LANE_END[int(si[s, SI["target_lane"]])] - 2.5
            if s >= n:
                f = int(z["hdv_front"][t, s])
                c["hdv_front_vehicle"] += int(f >= 0)
                c["hdv_front_none"] += int(f == -1)
                c["hdv_front_obstacle"] += int(f == -2)
                c["hdv_crashed_at_start"] += int(si[s, SI["crashed"]] != 0)
                c["follow_road_hdv"] += int(x > tl_end)
                continue
            c["key_ramp"] += int(lane == BC1)
            c["key_speed_le0"] += int(sf[s, SF["speed"]] <= 0)
            c["follow_road_cav"] += int(max(x, tr[s, T_EX]) > tl_end)
            c["live_crashed_ego"] += int(si[s, SI["crashed"]] != 0)
            a, tl = int(z["actions"][t, s]), int(si[s, SI["target_lane"]])
            if a in (0, 2):  # mdp_controller.py:37-48: only road (b, c) has a second lane to clip to
                c["lane_change_other_lane" if (a, tl) in ((0, BC1), (2, BC0)) else "lane_change_same_lane"] += 1
            ex = tr[s, T_EX]
            case = {BC0: "main_bc0", AB0: "main_ab0_ramp" if ex > 220.0 else "main_none", CD0: "main_none", BC1: "ramp_bc1",
                    KB0: "ramp_kb0", JK0: "ramp_none"}[lane]
            c["case_" + case] += 1
            crash = int(tr[s, T_CRASH])
            c["no_crash"] += int(crash < 0)
            h = int(z["hit"][t, s])
            if h >= 0:
                c[("hit_fl", "hit_rr", "hit_fr", "hit_rl", "hit_obstacle")[h]] += 1
            for o in tr[s, T_FL:T_RL + 1].astype(int):  # a neighbour that an earlier evaluation left at its crash-time point
                if 0 <= o < n and tr[o, T_CRASH] >= 0 and tr[o, T_POS] < tr[s, T_POS]:
                    c["crashed_standing_neighbour"] += 1
                    break
            if crash >= 0:
                new = int(z["new_actions"][t, s])
                if "replaced_by_%d" % new in c:
                    c["replaced_by_%d" % new] += 1
                rooms = tr[s, T_ROOM:T_ROOM + 5]
                rooms = rooms[~np.isnan(rooms)]
                c["room_tie"] += int((rooms == rooms.max()).sum() > 1)
    return c


def total_census(parts):
    tot = {k: 0 for k in CENSUS_REQUIRED}
    for p in parts:
        for k, v in p.items():
            tot[k] = tot.get(k, 0) + int(v)
    return tot


def left_only_scenes(seed, count):
    """Placed scenes of the one family the priority supervisor's placed states lack for dmc: a slow ramp-lane ego at the lowest
    speed index (SLOWER unavailable) with a faster HDV starting just behind it and ending ahead -- its front-right neighbour,
    behind it at the first points: every keep-lane room is negative and LANE_LEFT's is its absolute value.
    [("left_only", vehicles, actions)] in the form of supervisor_twin_util.placed_scenes."""
    import supervisor_twin_util as U
    rng = np.random.RandomState(seed)
    j = lambda a, b: float(rng.uniform(a, b))  # noqa: E731
    out = []
    for _ in range(count):
        x = j(335, 395)
        out.append(("left_only", [U._veh(x, 4.0, j(10, 12), target_speed=10.0, speed_index=0),
                                  U._veh(x - j(0.3, 1.5), 4.0 + j(-0.3, 0.3), j(22, 28), kind=2, target_speed=25.0)], [1]))
    return out


def faster_wins_scenes(seed, count):
    """Placed scenes in which FASTER is the replacement.  dmc re-applies the candidate at every sub-step, so for an ego that
    drives forward FASTER's first points are never behind IDLE's and its keep-lane rooms never larger.  It wins for a slow
    wrong-way ego (heading pi, moving towards -x) overlapping a reversing HDV at larger x that closes in on it: the HDV is its
    front-left neighbour, the gap shrinks point by point, and fleeing faster keeps more of it -- as long as the horizon is too
    short for the steering controller to turn the ego round, i.e. at n_step = 1 (3 points).
    [("faster_wins", vehicles, actions)] in the form of supervisor_twin_util.placed_scenes."""
    import supervisor_twin_util as U
    rng = np.random.RandomState(seed)
    j = lambda a, b: float(rng.uniform(a, b))  # noqa: E731
    out = []
    for _ in range(count):
        x, sp = j(120, 260), j(2, 6)
        out.append(("faster_wins", [U._veh(x, 0.0, sp, heading=np.pi + j(-0.01, 0.01), speed_index=int(rng.choice([1, 2, 3]))),
                                    U._veh(x + j(4.7, 5.2), 0.0, -(sp + j(6, 10)), kind=2, target_speed=20.0)], [int(rng.choice([1, 4]))]))
    return out


def tapes(prefix="dmc_"):
    return sorted(glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def natural_tapes():
    return tapes("dmc_v0_")


def load(path):
    z = np.load(path)
    return z, json.loads(str(z["meta"]))


def index():
    with open(os.path.join(GOLDEN, "dmc_index.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------------------------
# GPU plumbing
def make_env(E, N, ht, n_hdv=0, n_step=6, sim_freq=15, policy_freq=5, **kw):
    from marl_mass_amd import VecMergeEnv
    cfg = {"safety_guarantee": "dmc", "HEADWAY_TIME": ht, "action_masking": True, "n_step": n_step, "simulation_frequency": sim_freq,
           "policy_frequency": policy_freq}
    return VecMergeEnv(E, N, env_id="merge-multi-agent-v0", config=cfg, obs_f64=True, n_hdv=n_hdv, enable_dmc=True, **kw)


def tape_env(E, N, meta, **kw):
    return make_env(E, N, meta["headway_time"], n_hdv=min(meta["n_hdv"], 1) if N != meta["n"] + meta["n_hdv"] else meta["n_hdv"],
                    n_step=meta["n_step"], sim_freq=meta["simulation_frequency"], policy_freq=meta["policy_frequency"], **kw)


def force(env, sf, si, steps, n_merge):
    """Teacher forcing: the reference's state at the start of a step, one row per env ([E][N] rows, padded slots: kind 0)."""
    import torch
    from marl_mass_amd import _cabi as abi
    dev = env.device
    sf = np.nan_to_num(np.asarray(sf, dtype=np.float64))
    si = np.asarray(si)
    kind = si[..., SI["kind"]]
    hdv = kind == 2
    put = lambda plane, v: plane.copy_(torch.as_tensor(np.asarray(v), device=dev).to(plane.dtype))  # noqa: E731
    for name, col in (("X", "x"), ("Y", "y"), ("HEADING", "heading"), ("SPEED", "speed"), ("TARGET_SPEED", "target_speed")):
        put(env.f64[abi.F[name]], sf[..., SF[col]])
    # HDVs keep their last IDM action in the SAFE_* planes and the MOBIL timer in G_VX (mm_abi.h)
    put(env.f64[abi.F["SAFE_STEER"]], np.where(hdv, sf[..., SF["act_steer"]], 0.0))
    put(env.f64[abi.F["SAFE_ACC"]], np.where(hdv, sf[..., SF["act_acc"]], 0.0))
    put(env.f64[abi.F["G_VX"]], np.where(hdv, sf[..., SF["timer"]], np.where(kind == 1, np.nan, 0.0)))
    for name in ("LANE", "TARGET_LANE", "SPEED_INDEX", "CRASHED", "KIND"):
        put(env.u8[abi.B[name]], si[..., SI[name.lower()]])
    put(env.u8[abi.B["HL_ACTION"]], np.where(kind == 0, 0, 255))
    env.u8[abi.B["FLAGS"]].zero_()
    env.u8[abi.B["HIST_LEN"]].zero_()
    put(env.env_i32[abi.EP["STEPS"]], steps)
    put(env.env_i32[abi.EP["TIME"]], (meta_ratio(env)) * np.asarray(steps))
    put(env.env_i32[abi.EP["N_MERGE"]], n_merge)


def meta_ratio(env):
    return int(env.config["simulation_frequency"]) // int(env.config["policy_frequency"])


def assert_trace(got, want, what=""):
    """Trace integers exactly, trace floats within TOL (NaN where the reference has NaN)."""
    got, want = np.asarray(got), np.asarray(want)
    for k in TRACE_INT:
        bad = np.argwhere(got[..., k] != want[..., k])
        assert len(bad) == 0, "%s trace field %d differs at %s: device %s, reference %s" % (
            what, k, bad[:5].tolist(), got[..., k][tuple(bad[0])], want[..., k][tuple(bad[0])])
    for k in TRACE_FLOAT:
        g, w = got[..., k], want[..., k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), "%s trace field %d: NaN pattern differs" % (what, k)
        d = np.abs(np.nan_to_num(g) - np.nan_to_num(w))
        assert d.max(initial=0.0) <= TOL, "%s trace field %d off by %g at %s" % (what, k, d.max(), np.argwhere(d == d.max())[0].tolist())


def same_bits(a, b):
    """Bit-for-bit equality of two float64 tensors, NaNs included."""
    import torch
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
