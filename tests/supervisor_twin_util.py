"""What the supervisor-twin tests share (test_supervisor_twin_host.py on the CPU, test_supervisor_twin_gpu.py on the MI355X,
tools/supervisor_ref_fuzz.py against the reference): states as plain arrays and how to put them into an env of either
backend, the twin's trace and census, the device kernel's lookahead copy read back from its scratch buffer, the seeded
generator of placed rare-branch states, and the supervisor's Philox uniforms from the numpy Philox of policy_act_util.

The chain is  reference -> twin (oracle/mm_oracle.c mm_supervise, CPU) -> kernel (mm_supervisor.hip, GPU):  the twin is pinned
to the reference by the prio_* / sup_placed_* tapes and tools/supervisor_ref_fuzz.py, the kernel to the twin bit for bit in
math mode 1.  A plain module: nothing here touches the GPU unless it is handed device tensors."""
import ctypes as C
import glob
import json
import os

import numpy as np
import torch

from marl_mass_amd import _cabi as abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-9
SUP_DOMAIN = 0x53555056  # the domain word of the supervisor's Philox draws (include/mm_supervisor.h)
LIVE = ("x", "y", "heading", "speed", "target_speed", "target_lane", "crashed", "hdv_steer", "hdv_acc")
# columns of sub_f / sub_i (tools/gen_golden._veh_snapshot)
SF = {"x": 0, "y": 1, "heading": 2, "speed": 3, "target_speed": 4, "act_steer": 5, "act_acc": 6, "timer": 10}
SI = {"lane": 0, "target_lane": 1, "speed_index": 2, "crashed": 3, "kind": 8}
AB0, BC0, BC1, CD0, JK0, KB0 = range(6)
F_KEYS = ("x", "y", "heading", "speed", "target_speed")
I_KEYS = ("lane", "target_lane", "speed_index", "crashed", "kind")

# Census entries (oracle/mm_oracle.c sup_census_names) the GPU tests require at least CENSUS_MIN times over the union of their
# free-run and placed inputs, counted by the TWIN on the CPU.  "replaced_by_2" is not in the list: LANE_RIGHT is never an
# available action -- _get_available_actions (abstract.py:229-235) offers it only on a lane with a higher-numbered side lane
# that is_reachable_from the vehicle, the only such side lane is (b, c, 1), and that lane is forbidden (merge_env_v1.py
# lane table), so is_reachable_from (lane.py:78-90) is False for every position.  No state, placed or natural, reaches it.
CENSUS_MIN = 20
CENSUS_REQUIRED = (
    "key_ramp", "key_speed_le0", "key_no_front", "key_next_lane_headway", "order_differs",
    "ego_reset", "neighbour_skipped",
    "query_bc0_bc1", "query_ab0_kb0", "query_kb0_ab0", "query_bc1_bc0", "query_none",
    "follow_road_cav", "follow_road_hdv", "lane_change_accepted", "lane_change_refused",
    "hdv_front_vehicle", "hdv_front_none", "hdv_front_obstacle", "hdv_crashed_start",
    "speed_clip_cav", "speed_clip_hdv",
    "collision_fl", "collision_rl", "collision_fr", "collision_rr", "collision_obstacle", "collision_min_ego", "collision_min_other",
    "replaced_by_0", "replaced_by_1", "replaced_by_3", "replaced_by_4",
    "second_replacement", "room_tie", "neighbour_crash_cleared", "ego_crashed_start",
)
FREE_RUN_MIN_REPLACED = 500


def oracle():
    from oracle import oracle_env
    return oracle_env


# ---------------------------------------------------------------------------------------------------------------------
# tapes
def tapes(prefix):
    return sorted(glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def replay_tapes():
    """Every tape the twin tests replay: the natural prio_v0_* episodes, the adapter's tape and the placed rare-branch ones."""
    return tapes("prio_v0_") + tapes("prio_compat_") + tapes("sup_placed_")


def load_tape(path):
    z = np.load(path)
    return z, json.loads(str(z["meta"]))


def tape_state(z, rows=slice(None)):
    """The state of the recorded steps `rows` as the arrays put_state takes ([T][m] each)."""
    sf, si = np.nan_to_num(z["sub_f"][rows]), z["sub_i"][rows]
    st = {k: sf[..., SF[k]].copy() for k in F_KEYS}
    st.update({k: si[..., SI[k]].astype(np.int64) for k in I_KEYS})
    st["act_steer"], st["act_acc"], st["timer"] = sf[..., SF["act_steer"]], sf[..., SF["act_acc"]], sf[..., SF["timer"]]
    return st


def tape_config(meta):
    cfg = {"safety_guarantee": "priority", "HEADWAY_TIME": meta["headway_time"], "action_masking": True,
           "n_step": meta.get("n_step", 6)}
    if "simulation_frequency" in meta:
        cfg["simulation_frequency"] = meta["simulation_frequency"]
    return cfg


# ---------------------------------------------------------------------------------------------------------------------
# states
def pad_state(st, N):
    """The same rows in N slots: absent slots (kind 0, every plane zero) follow the vehicles."""
    out = {}
    for k, v in st.items():
        v = np.asarray(v)
        w = np.zeros((v.shape[0], N), dtype=v.dtype)
        w[:, :v.shape[1]] = v
        out[k] = w
    return out


def cat_states(states):
    return {k: np.concatenate([s[k] for s in states], axis=0) for k in states[0]}


def put_state(env, st, steps=0, n_merge=0, episode=None):
    """Teacher forcing on either backend: every plane the supervisor and the step read, one row per env ([E][N] arrays, absent
    slots: kind 0).  HDVs keep their last IDM action in the SAFE_* planes and the MOBIL timer in G_VX (mm_abi.h)."""
    dev = env.device
    put = lambda plane, v: plane.copy_(torch.as_tensor(np.array(v), device=dev).to(plane.dtype))  # noqa: E731
    hdv = np.asarray(st["kind"]) == 2
    zero = np.zeros(hdv.shape)
    for name, key in (("X", "x"), ("Y", "y"), ("HEADING", "heading"), ("SPEED", "speed"), ("TARGET_SPEED", "target_speed")):
        put(env.f64[abi.F[name]], st[key])
    put(env.f64[abi.F["SAFE_STEER"]], np.where(hdv, st.get("act_steer", zero), 0.0))
    put(env.f64[abi.F["SAFE_ACC"]], np.where(hdv, st.get("act_acc", zero), 0.0))
    put(env.f64[abi.F["G_VX"]], np.where(hdv, st.get("timer", zero), np.where(np.asarray(st["kind"]) == 1, np.nan, 0.0)))
    for name in ("LANE", "TARGET_LANE", "SPEED_INDEX", "CRASHED", "KIND"):
        put(env.u8[abi.B[name]], st[name.lower()])
    env.u8[abi.B["HL_ACTION"]].copy_(torch.as_tensor(np.where(np.asarray(st["kind"]) == 0, 0, 255), device=dev).to(torch.uint8))
    env.u8[abi.B["FLAGS"]].zero_()
    env.u8[abi.B["HIST_LEN"]].zero_()
    E = env.E
    put(env.env_i32[abi.EP["STEPS"]], np.broadcast_to(np.asarray(steps), (E,)))
    put(env.env_i32[abi.EP["TIME"]], 3 * np.broadcast_to(np.asarray(steps), (E,)))
    put(env.env_i32[abi.EP["N_MERGE"]], np.broadcast_to(np.asarray(n_merge), (E,)))
    if episode is not None:
        put(env.env_i32[abi.EP["EPISODE"]], np.broadcast_to(np.asarray(episode), (E,)))


# ---------------------------------------------------------------------------------------------------------------------
# the twin's trace and census
class Trace(object):
    """The twin's report of one mm_supervise call (orc_supervise_trace): per env the priority order and numbers, per vehicle
    the final lookahead copy -- len(trajectories), the live fields LIVE, and every stored point (x, y, heading, speed; x = y =
    NaN for the aliased point of a crashed HDV)."""

    def __init__(self, E, N, n_points):
        self.E, self.N, self.n_points = E, N, n_points
        self.buf = np.zeros((E, N * (2 + 10 + 4 * n_points)))

    def __enter__(self):
        oracle().library().lib.orc_supervise_trace(self.buf.ctypes.data, self.buf.size)
        return self

    def __exit__(self, *a):
        oracle().library().lib.orc_supervise_trace(None, 0)

    def parse(self):
        E, N, P = self.E, self.N, self.n_points
        veh = self.buf[:, 2 * N:].reshape(E, N, 10 + 4 * P)
        return {"order": self.buf[:, :N].astype(np.int64), "key": self.buf[:, N:2 * N].copy(), "len": veh[:, :, 0].astype(np.int64),
                "live": veh[:, :, 1:10].copy(), "points": veh[:, :, 10:].reshape(E, N, P, 4).copy()}


def scratch_copy(scratch, E, N, n_points):
    """The device kernel's lookahead copy, read back from its scratch buffer after the call.  The layout is the View struct of
    mm_supervisor.hip: kLive = 10 live fields (x, y, heading, speed, target speed, target lane, crashed, len(trajectories), HDV
    steering, HDV acceleration), then [point][4] (x, y, heading, speed), every one a plane [.][slot][env].  Returned in the
    Trace.parse() arrangement.  Only vehicles with at least one point are specified; the rest of the scratch is not."""
    s = scratch[: E * N * (10 + 4 * n_points)].detach().cpu().numpy().reshape(10 + 4 * n_points, N, E)
    live = s[:10].transpose(2, 1, 0)  # [E][N][10]
    pts = s[10:].reshape(n_points, 4, N, E).transpose(3, 2, 0, 1)  # [E][N][P][4]
    return {"len": live[:, :, 7], "live": np.concatenate([live[:, :, :7], live[:, :, 8:10]], axis=2), "points": pts}


def same_bits(a, b):
    """Equality of every bit of two float64 arrays, NaN payloads aside (a NaN equals a NaN)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def assert_copy_equal(tw, dev, what=""):
    """The twin's trace against the kernel's scratch: for every vehicle the twin stepped (>= 1 point) the same point count,
    live fields and points, bit for bit."""
    has = tw["len"] > 0
    dlen = np.where(has, dev["len"], 0)
    assert np.array_equal(dlen, np.where(has, tw["len"], 0)), what + ": point counts differ at %s" % (np.argwhere(dlen != tw["len"])[:5].tolist(),)
    ok = same_bits(tw["live"], dev["live"]) | ~has[:, :, None]
    assert ok.all(), what + ": live fields differ at [env, slot, field] %s" % (np.argwhere(~ok)[:5].tolist(),)
    P = tw["points"].shape[2]
    used = np.arange(P)[None, None, :] < tw["len"][:, :, None]
    okp = same_bits(tw["points"], dev["points"]) | ~used[..., None]
    assert okp.all(), what + ": points differ at [env, slot, point, field] %s" % (np.argwhere(~okp)[:5].tolist(),)
    return int(has.sum())


def census_names():
    lib = oracle().library().lib
    n = lib.orc_supervise_census(None, 0)
    return [lib.orc_supervise_census_name(k).decode() for k in range(n)]


def census():
    """Branch counters of the twin's last mm_supervise call, summed over its envs."""
    lib = oracle().library().lib
    names = census_names()
    out = (C.c_int64 * len(names))()
    lib.orc_supervise_census(out, len(names))
    return dict(zip(names, [int(x) for x in out]))


def add_census(total, c):
    for k, v in c.items():
        total[k] = total.get(k, 0) + v
    return total


# ---------------------------------------------------------------------------------------------------------------------
# the supervisor's Philox uniforms from an outside implementation
def philox_uniforms(seeds, episode, steps, n):
    """uniforms[e][d] = draw d of env e as include/mm_supervisor.h documents it: Philox4x32-10 with the counter (d, MM_E_EPISODE,
    MM_E_STEPS, domain word) and the env's seed as the key, u53 of output words 0 and 1 -- from the numpy Philox of
    policy_act_util (pinned to the published known answers there)."""
    from policy_act_util import philox4x32_10, u53
    seeds, episode, steps = np.asarray(seeds), np.asarray(episode), np.asarray(steps)
    U = np.zeros((len(seeds), n))
    d = np.arange(n)
    for e in range(len(seeds)):
        s = int(seeds[e]) & ((1 << 64) - 1)
        w = philox4x32_10((d, int(episode[e]) & 0xFFFFFFFF, int(steps[e]) & 0xFFFFFFFF, SUP_DOMAIN), (s & 0xFFFFFFFF, s >> 32))
        U[e] = u53(w[0], w[1])
    return U


# ---------------------------------------------------------------------------------------------------------------------
# placed states: built to reach the branches natural episodes rarely or never do
def _closest_lane(x, y, h):
    lib = oracle().library().lib
    return int(lib.orc_closest_lane(float(x), float(y), float(h)))


def _speed_index(target_speed):
    return int(np.clip(np.rint((target_speed - 10.0) / 20.0 * 4), 0, 4))


def _veh(x, y, speed, kind=1, heading=0.0, target_speed=None, crashed=0, speed_index=None, target_lane=None):
    lane = _closest_lane(x, y, heading)
    ts = speed if target_speed is None else target_speed
    si = (_speed_index(ts) if speed_index is None else speed_index) if kind == 1 else 0
    return dict(x=x, y=y, heading=heading, speed=speed, target_speed=ts, lane=lane, target_lane=lane if target_lane is None else target_lane,
                speed_index=si, crashed=crashed, kind=kind)


def _scene(rng, family):
    """One placed scene: (vehicles, CAVs first; actions of the CAVs).  j(a, b) jitters every number so that no two scenes of a
    family are alike."""
    j = lambda a, b: float(rng.uniform(a, b))  # noqa: E731
    C_, H_ = 1, 2
    if family == "obstacle":  # ego on the ramp lane short of its end: runs into the obstacle; an HDV behind sees the obstacle
        x = j(398, 414)       # ahead once the ego is its neighbour, a main-road CAV alongside has the HDV as ramp neighbour
        return [_veh(x, 4.0 + j(-0.2, 0.2), j(22, 30)), _veh(x - j(30, 50), 0.0, j(20, 25)),
                _veh(x + j(18, 25), 4.0, j(0, 3), kind=H_, target_speed=j(20, 30))], [int(rng.choice([1, 3])), int(rng.choice([1, 3, 4]))]
    if family == "obstacle_hdv":  # an HDV alone on the ramp lane ahead of the obstacle, its CAV neighbour on the main lane
        x = j(340, 400)
        return [_veh(x + j(-10, 10), 0.0, j(20, 28)), _veh(x, 4.0, j(15, 25), kind=H_, target_speed=j(20, 30))], [int(rng.choice([0, 1, 2, 3, 4]))]
    if family == "speeds":  # a stopped CAV, one above MAX_SPEED, an HDV above MAX_SPEED, on the main road
        x = j(40, 150)
        return [_veh(x, 0.0, 0.0 if rng.rand() < 0.7 else -j(0, 2), target_speed=j(10, 30)), _veh(x + j(25, 40), 0.0, j(40.5, 46), target_speed=30.0),
                _veh(x - j(40, 70), 0.0, j(40.5, 47), kind=H_, target_speed=j(25, 30)),
                _veh(x + j(50, 90), 0.0, j(41, 44), kind=H_, target_speed=30.0)], [int(rng.choice([1, 3, 4])), int(rng.choice([1, 3, 4]))]
    if family == "crashed_hdv":  # a crashed HDV just ahead of the ego on its lane: its points alias its position, and it moves
        main = rng.rand() < 0.5  # again once a replacement clears the flag
        x, y = (j(60, 280), 0.0) if main else (j(330, 380), 4.0)
        return [_veh(x, y, j(18, 30)), _veh(x - j(20, 40), y, j(20, 28)),
                _veh(x + j(5.2, 9.0), y, j(0, 12), kind=H_, crashed=1, target_speed=j(20, 30)),
                _veh(x + j(40, 60), y, j(20, 25), kind=H_, crashed=int(rng.rand() < 0.5), target_speed=25.0)], [int(rng.choice([1, 3])), int(rng.choice([1, 3, 4]))]
    if family == "crashed_ego":  # the ego is crashed when the call starts: replaced at every sub-step; alone, every room ties
        x = j(30, 280)
        vs = [_veh(x, 0.0, j(5, 25), crashed=1, target_speed=j(15, 25))]
        if rng.rand() < 0.5:
            vs.append(_veh(x + j(70, 120), 0.0, j(20, 30)))
        return vs, [int(rng.choice([0, 1, 2, 3, 4])) for _ in vs]
    if family == "four_slots_main":  # main-road ego between a slow leader and a fast follower: front-left / rear-left collisions
        x = j(60, 250)
        front = rng.rand() < 0.5
        vs = [_veh(x, 0.0, j(24, 30) if front else j(10, 14)),
              _veh(x + (j(5.5, 8) if front else j(40, 60)), 0.0, j(8, 12) if front else j(20, 25), kind=int(rng.choice([C_, H_])), target_speed=20.0),
              _veh(x - (j(40, 60) if front else j(5.5, 8)), 0.0, j(20, 24) if front else j(27, 33), kind=int(rng.choice([C_, H_])), target_speed=30.0)]
        vs.sort(key=lambda v: v["kind"])
        n = sum(1 for v in vs if v["kind"] == C_)
        return vs, [int(rng.choice([1, 3])) for _ in range(n)]
    if family == "four_slots_ramp":  # the same on the ramp (kb0 / bc1): front-right / rear-right collisions
        x = j(330, 390) if rng.rand() < 0.6 else j(150, 210)
        y = 4.0 if x > 320 else 10.5
        front = rng.rand() < 0.5
        vs = [_veh(x, y, j(24, 30) if front else j(10, 14)),
              _veh(x + (j(5.5, 8) if front else j(40, 60)), y, j(8, 12) if front else j(20, 25), kind=int(rng.choice([C_, H_])), target_speed=20.0),
              _veh(x - (j(40, 60) if front else j(5.5, 8)), y, j(20, 24) if front else j(27, 33), kind=int(rng.choice([C_, H_])), target_speed=30.0),
              _veh(x + j(-20, 20), 0.0, j(20, 25))]
        vs.sort(key=lambda v: v["kind"])
        n = sum(1 for v in vs if v["kind"] == C_)
        return vs, [int(rng.choice([1, 3])) for _ in range(n)]
    if family == "left_wins":  # ramp-lane ego overlapping a slower vehicle whose centre it passes at once: every keep-lane room is
        x = j(335, 400)        # negative, LANE_LEFT's is its absolute value
        return [_veh(x, 4.0, j(26, 30)), _veh(x + j(0.05, 1.2), 4.0 + j(-0.3, 0.3), j(5, 10), kind=int(rng.choice([C_, H_])), target_speed=10.0)], \
            [int(rng.choice([1, 3])), 1]
    if family == "wrong_way":  # an ego heading against the road, fleeing a reversing HDV that its query calls its front vehicle:
        x = j(120, 260)        # the gap shrinks with time and FASTER keeps more of it than IDLE -- the one way FASTER can win
        return [_veh(x, 0.0, j(12, 18), heading=np.pi + j(-0.01, 0.01), speed_index=int(rng.choice([1, 2, 3]))),
                _veh(x + j(7.5, 9.5), 0.0, -j(30, 38), kind=H_, target_speed=20.0)], [int(rng.choice([1, 4]))]
    if family == "lane_ends":  # vehicles past the end of their target lane: follow_road switches it inside the lookahead
        vs = [_veh(j(317.6, 319.5), 0.0, j(20, 28)), _veh(j(280, 300), 0.0, j(20, 28)), _veh(j(217.6, 219.8), 10.5, j(20, 28)),
              _veh(j(317.6, 319.9), 4.0 + j(-0.1, 0.1), j(20, 26), kind=H_, target_speed=25.0, target_lane=KB0),
              _veh(j(417.6, 419.9), 0.0, j(20, 26), kind=H_, target_speed=25.0, target_lane=BC0),
              _veh(j(330, 345), 0.0, j(20, 26), kind=H_, target_speed=25.0)]
        return vs, [int(rng.choice([0, 1, 2, 3, 4])) for _ in range(3)]
    raise KeyError(family)


FAMILIES = ("obstacle", "obstacle_hdv", "speeds", "crashed_hdv", "crashed_ego", "four_slots_main", "four_slots_ramp", "left_wins",
            "wrong_way", "lane_ends")


def placed_scenes(seed, per_family=40):
    """[(family, vehicles, actions)] regenerated from the seed; CAVs first in every scene."""
    rng = np.random.RandomState(seed)
    out = []
    for fam in FAMILIES:
        for _ in range(per_family):
            vs, acts = _scene(rng, fam)
            vs = sorted(vs, key=lambda v: v["kind"])  # (stable: CAVs keep their order, then the HDVs)
            n = sum(1 for v in vs if v["kind"] == 1)
            assert len(acts) >= n
            out.append((fam, vs, list(acts[:n])))
    return out


def scenes_to_state(scenes, N, seed=0):
    """The scenes as one batch of N slots: (state, actions [E][N]).  Slots past a scene's vehicles are absent; their action
    codes, and those of HDV slots, are arbitrary (they pass through).  On top come rows with no controlled vehicle (empty, and
    HDVs only) and, on every fourth scene, action codes outside 0..4 on a controlled vehicle."""
    rng = np.random.RandomState(seed + 17)
    rows, acts = [], []
    for k, (fam, vs, a) in enumerate(scenes):
        assert len(vs) <= N
        row = {key: np.zeros(N) for key in F_KEYS}
        row.update({key: np.zeros(N, dtype=np.int64) for key in I_KEYS})
        for s, v in enumerate(vs):
            for key in F_KEYS + I_KEYS:
                row[key][s] = v[key]
        act = rng.randint(-3, 9, size=N).astype(np.int32)
        act[:len(a)] = a
        if k % 4 == 3:
            act[int(rng.randint(len(a)))] = int(rng.choice([-1, 5, 7, 100]))
        rows.append(row)
        acts.append(act)
    for hdv_only in (0, 1, 1):  # rows with no controlled vehicle
        row = {key: np.zeros(N) for key in F_KEYS}
        row.update({key: np.zeros(N, dtype=np.int64) for key in I_KEYS})
        if hdv_only:
            for s in range(2):
                v = _veh(float(rng.uniform(50, 300)) + 40 * s, 0.0, 22.0, kind=2, target_speed=25.0)
                for key in F_KEYS + I_KEYS:
                    row[key][s] = v[key]
        rows.append(row)
        acts.append(rng.randint(-3, 9, size=N).astype(np.int32))
    st = {key: np.stack([r[key] for r in rows]) for key in F_KEYS + I_KEYS}
    return st, np.stack(acts)
