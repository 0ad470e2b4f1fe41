"""The tapes of tests/test_candidate_prior_gpu.py, and what they must contain (CPU, oracle only).

step_kernel's kPrimary kernels predict, in the main pass, the candidate the veto prior picks: B (steer to the current lane)
for a vehicle with needB whose MM_FLAG_IS_LC_SAFE is clear, else A (steer to the target lane); the other candidate is
evaluated where it is first read.  The parity test can only catch a mistake in a case that its tapes contain, so the cases
are counted here, from the oracle's per-sub-step trace alone (math mode 1), per vehicle and sub-step:

  P1  first_B and the veto holds: A is never needed
  P2  first_B and the veto is lifted in that sub-step: A is needed lazily
  P3  needB, prior "safe", and the veto fires: B is needed lazily
  P4  a crashed vehicle whose shield runs (crashed => needB), under either prior

with  ran     = the shield ran for the vehicle in that sub-step (QP_ROWS > 0),
      needB   = ran and (target lane after act != lane  or  crashed),
      first_B = needB and not (flags before the sub-step & IS_LC_SAFE),
      veto    = ran and not (flags after the sub-step & IS_LC_SAFE)      (shield_post: IS_LC_SAFE is set iff no veto).

The target lane after act is not in the trace where a veto fired (the commit resets it to the lane), so act's lane logic
(follow_road, the LEFT / RIGHT request; controller.py:90-144) is replayed here on the oracle's own lane functions, and the
replay is checked against the trace wherever no veto fired.

An episode ends with the sub-step in which a vehicle crashes, so the random tapes hold no P4: the "crash" tape scripts it --
after three steps of the 9 x 8 tape the caller marks some vehicles crashed in the state planes, and the next step's first
sub-step runs their shields.  The small shapes' random tapes hold no P2 (their traffic is sparse and a lifted veto is rare):
the "unsafe" tapes script it for them -- over forty steps in the merging zone the caller clears IS_LC_SAFE on every vehicle
before each step, so the prior picks B for every lane change under way, and the shields lift most of these vetoes at once.
The counts P1 - P3 are asserted on the random tapes alone.
"""
import ctypes as C
import functools

import torch

import oracle_env
from marl_mass_amd import _cabi as abi

SHAPES = {"E9_N8": (9, 8), "E5_N4": (5, 4), "E3_N2": (3, 2), "E5_N5": (5, 5)}
SHIELDS = {"mass": "cbf-cav", "hss": "cbf-av"}
STEPS = 120
TAPE_SEED = 31
# lane-change-heavy and accelerating (LEFT, IDLE, RIGHT, FASTER, SLOWER): closing gaps make vetoes fire and lift; of the mixes and
# seeds tried, this one holds the rare cases (P2, P3) most often
P_ACT = torch.tensor([0.3, 0.1, 0.3, 0.25, 0.05])
CRASH_AFTER = 3  # the crash tape: steps before the caller's edit
UNSAFE_FROM, UNSAFE_TO = 40, 80  # the "unsafe" tapes: the caller clears IS_LC_SAFE before each of these steps
UNSAFE_SHAPES = ("E5_N4", "E3_N2")
CRASH_SLOTS = ((0, 0), (1, 3), (2, 5), (4, 1), (4, 6), (6, 2), (8, 7), (8, 0))  # (env, vehicle) marked crashed, 9 x 8

AB0, BC0, BC1, CD0, JK0, KB0 = (abi.LANE_ID[l] for l in abi.LANE_INDEX)
ROAD = {AB0: 0, BC0: 1, BC1: 1, CD0: 2, JK0: 3, KB0: 4}


def kw(shield, seed=4242, **more):
    d = dict(env_id="merge-multi-agent-v1", config={"safety_guarantee": SHIELDS[shield], "HEADWAY_TIME": 0.5},
             cbf_eta=0.03125, cbf_tau=0.5, qp_solver="exact", obs_f64=True, auto_reset=True, seed=seed)
    d.update(more)
    return d


def actions(E, N, steps, seed=TAPE_SEED):
    g = torch.Generator().manual_seed(seed)
    return [torch.multinomial(P_ACT, E * N, True, generator=g).view(E, N).int() for _ in range(steps)]


def snap(env, step_result):
    obs, rew, done, info = step_result
    rec = {"f64": env.f64, "u8": env.u8, "env_i32": env.env_i32, "obs": obs, "reward": rew, "done": done}
    rec.update({"info." + k: w for k, w in info.items()})
    return {k: w.detach().cpu().clone() for k, w in rec.items()}


def same(a, b):
    if a.is_floating_point():
        return torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)) and torch.equal(a.isnan(), b.isnan())
    return torch.equal(a, b)


def assert_same(got, want, where):
    assert set(got) == set(want), where
    for k in sorted(want):
        assert same(got[k], want[k]), (where, k)


def mark_crashed(env):
    """The caller's edit of the crash tape: CRASH_SLOTS become crashed vehicles (state planes, env's own device)."""
    for e, v in CRASH_SLOTS:
        env.u8[abi.B["CRASHED"], e, v] = 1


def _pre(env):
    return {"u8": env.u8.clone(), "f64": env.f64[:2].clone(), "time": env.env_i32[abi.EP["TIME"]].clone()}


@functools.lru_cache(maxsize=None)
def oracle_tape(shape, shield):
    """The oracle's run of a case, once: per step the record the GPU is compared with, the state before it and the trace."""
    E, N = SHAPES[shape]
    oracle_env.set_math_mode(1)  # include/mm_math.h on both sides: bit-for-bit comparison
    try:
        env = oracle_env.OracleEnv(E, N, trace=True, **kw(shield))
        env.reset()
        tape = []
        for a in actions(E, N, STEPS):
            pre = _pre(env)
            rec = snap(env, env.step(a))
            tape.append({"rec": rec, "pre": pre, "trace": env.trace.clone(), "act": a})
        return tape
    finally:
        oracle_env.set_math_mode(0)


def mark_unsafe(env):
    """The caller's edit of the "unsafe" tapes: IS_LC_SAFE cleared on every vehicle, as if every last decision had been a veto.
    The prior then picks B for every vehicle with a lane change under way, and most of these vetoes are lifted at once."""
    env.u8[abi.B["FLAGS"]] &= 0xFF ^ abi.FLAG_IS_LC_SAFE


@functools.lru_cache(maxsize=None)
def oracle_crash_tape(shield):
    """CRASH_AFTER steps of the 9 x 8 tape, the caller's edit (mark_crashed), one more step."""
    E, N = SHAPES["E9_N8"]
    oracle_env.set_math_mode(1)
    try:
        env = oracle_env.OracleEnv(E, N, trace=True, **kw(shield))
        env.reset()
        acts = actions(E, N, CRASH_AFTER + 1)
        for a in acts[:-1]:
            env.step(a)
        mark_crashed(env)
        pre = _pre(env)
        rec = snap(env, env.step(acts[-1]))
        return [{"rec": rec, "pre": pre, "trace": env.trace.clone(), "act": acts[-1]}]
    finally:
        oracle_env.set_math_mode(0)


@functools.lru_cache(maxsize=None)
def oracle_unsafe_tape(shape, shield):
    """The shape's tape up to UNSAFE_TO, with the caller's edit (mark_unsafe) before each step from UNSAFE_FROM on: those steps."""
    E, N = SHAPES[shape]
    oracle_env.set_math_mode(1)
    try:
        env = oracle_env.OracleEnv(E, N, trace=True, **kw(shield))
        env.reset()
        tape = []
        for t, a in enumerate(actions(E, N, UNSAFE_TO)):
            if t < UNSAFE_FROM:
                env.step(a)
                continue
            mark_unsafe(env)
            pre = _pre(env)
            rec = snap(env, env.step(a))
            tape.append({"rec": rec, "pre": pre, "trace": env.trace.clone(), "act": a})
        return tape
    finally:
        oracle_env.set_math_mode(0)


def _lane_fns():
    lib = oracle_env.library().lib
    after_end = lambda l, x, y: bool(lib.orc_after_end(l, x, y))  # noqa: E731
    reachable = lambda l, x, y: bool(lib.orc_is_reachable_from(l, x, y))  # noqa: E731
    nxt = lambda l, x, y: int(lib.orc_next_lane(l, C.c_double(x), C.c_double(y)))  # noqa: E731
    return after_end, reachable, nxt


def _target_after_act(fns, tl, x, y, action, high_level):
    """ControlledVehicle.act's lane logic: MDPVehicle.act(action) where the policy acts, then road.act's act(None)."""
    after_end, reachable, nxt = fns

    def follow(t):
        return nxt(t, x, y) if after_end(t, x, y) else t

    if high_level:
        tl = follow(tl)
        if action in (0, 2):
            cand = (BC1 if action == 2 else BC0) if ROAD[tl] == 1 else tl
            if reachable(cand, x, y):
                tl = cand
    return follow(tl)


def count_cases(tape, N):
    """{"P1": [sub-step 0, later], "P2": .., "P3": .., "P4": n} over a tape, and the number of replay checks made."""
    fns = _lane_fns()
    T, B, SAFE = abi.T, abi.B, abi.FLAG_IS_LC_SAFE
    n = {"P1": [0, 0], "P2": [0, 0], "P3": [0, 0], "P4": 0, "replayed": 0}
    for st in tape:
        tr, pre, act = st["trace"], st["pre"], st["act"]
        nsub = tr.shape[0]
        E = tr.shape[2]
        for e in range(E):
            for v in range(N):
                if int(pre["u8"][B["KIND"], e, v]) == 0:
                    continue
                lane, tl = int(pre["u8"][B["LANE"], e, v]), int(pre["u8"][B["TARGET_LANE"], e, v])
                crashed, flags = int(pre["u8"][B["CRASHED"], e, v]), int(pre["u8"][B["FLAGS"], e, v])
                x, y = float(pre["f64"][abi.F["X"], e, v]), float(pre["f64"][abi.F["Y"], e, v])
                for k in range(nsub):
                    t = tr[k, :, e, v]
                    if bool(torch.isnan(t[T["X"]])):
                        break  # the episode ended in an earlier sub-step
                    hl = (int(pre["time"][e]) + k) % nsub == 0
                    tl_act = _target_after_act(fns, tl, x, y, int(act[e, v]), hl)
                    ran = float(t[T["QP_ROWS"]]) > 0
                    flags_post = int(t[T["FLAGS"]])
                    veto = ran and not (flags_post & SAFE)
                    if not veto:  # the commit leaves the target lane alone: the replay must agree with the oracle
                        assert tl_act == int(t[T["TARGET_LANE"]]), ("target-lane replay", e, v, k)
                        n["replayed"] += 1
                    else:
                        assert int(t[T["TARGET_LANE"]]) == lane, ("a veto re-targets the current lane", e, v, k)
                    need_b = ran and (tl_act != lane or crashed != 0)
                    first_b = need_b and not (flags & SAFE)
                    pos = 0 if k == 0 else 1
                    if first_b and veto:
                        n["P1"][pos] += 1
                    if first_b and not veto:
                        n["P2"][pos] += 1
                    if need_b and (flags & SAFE) and veto:
                        n["P3"][pos] += 1
                    if ran and crashed:
                        n["P4"] += 1
                    lane, tl, crashed, flags = int(t[T["LANE"]]), int(t[T["TARGET_LANE"]]), int(t[T["CRASHED"]]), flags_post
                    x, y = float(t[T["X"]]), float(t[T["Y"]])
    return n


@functools.lru_cache(maxsize=None)
def totals():
    """The cases over the random tapes of the GPU test's new-path shapes (2-, 4-, 8-lane groups) and the crash tapes; per tape, the
    "unsafe" tapes too."""
    tot = {"P1": [0, 0], "P2": [0, 0], "P3": [0, 0], "P4": 0, "replayed": 0}
    per = {}
    for shield in SHIELDS:
        for shape in ("E9_N8", "E5_N4", "E3_N2"):
            per[shape, shield] = count_cases(oracle_tape(shape, shield), SHAPES[shape][1])
        per["crash", shield] = count_cases(oracle_crash_tape(shield), 8)
        for shape in UNSAFE_SHAPES:
            per["unsafe " + shape, shield] = count_cases(oracle_unsafe_tape(shape, shield), SHAPES[shape][1])
    for key, c in per.items():
        tot["replayed"] += c["replayed"]
        if key[0].startswith("unsafe"):
            continue  # (scripted on top: what the counts ask for is met without them)
        for p in ("P1", "P2", "P3"):
            tot[p][0] += c[p][0]
            tot[p][1] += c[p][1]
        tot["P4"] += c["P4"]
    return tot, per


def test_the_tapes_contain_every_case():
    tot, per = totals()
    print("candidate-prior cases in the tapes:", tot)
    for key in sorted(per):
        print("  ", key, per[key])
    assert tot["replayed"] > 1000  # the replay of act's lane logic was checked against the oracle throughout
    for p in ("P1", "P2", "P3"):
        assert tot[p][0] >= 10, (p, "sub-step 0", tot[p])
        assert tot[p][1] >= 10, (p, "later sub-steps", tot[p])
    assert tot["P4"] >= 3, tot["P4"]


def test_each_shield_meets_every_case_in_the_widest_group():
    """MASS and HSS are kernels of their own: the 9 x 8 tape of each holds every case in either position a few times (3: more
    than a single coincidence), and the crash tape of each its crashed vehicles."""
    _, per = totals()
    for shield in SHIELDS:
        c = per["E9_N8", shield]
        for p in ("P1", "P2", "P3"):
            assert c[p][0] >= 3 and c[p][1] >= 3, (shield, p, c[p])
        assert per["crash", shield]["P4"] >= 3, (shield, per["crash", shield])


def test_the_unsafe_tapes_lift_vetoes_in_every_group_size():
    """The 4- and 2-lane kernels of either shield evaluate A lazily a few times (3: more than a single coincidence): a first_B
    lane whose veto is lifted.  (The 8-lane kernels: the random tape, above.)"""
    _, per = totals()
    for shield in SHIELDS:
        for shape in UNSAFE_SHAPES:
            assert per["unsafe " + shape, shield]["P2"][0] >= 3, (shape, shield, per["unsafe " + shape, shield])


def test_every_env_respawns_in_the_tapes():
    for shield in SHIELDS:
        for shape in SHAPES:
            tape = oracle_tape(shape, shield)
            assert bool(torch.stack([s["rec"]["done"] for s in tape]).any(0).all()), (shape, shield)
