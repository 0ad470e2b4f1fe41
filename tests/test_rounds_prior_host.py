"""The MASS rounds of step_kernel reach the same answer from the seed 0.0 and from the seed of MM_ROUNDS_PRIOR (CPU, oracle only).

The exact-mode MASS kernels find the accelerations the vehicles of an env DECIDE in a sub-step by iterating: every lane
evaluates its QP from the decisions its leader / front-adjacent vehicle currently shows, until no lane changes.  With
MM_ROUNDS_PRIOR a shielded lane starts from the acceleration of its inactive QP, (u0 - evx) / dt, instead of 0.0.  This file
replays that loop in Python floats -- the expressions of slot_gu, shield_rows, qp_exact and div_c (the correctly rounded
quotient, `/` here), IEEE doubles without contraction as the kernels are built -- on records taken from the oracle's trace
of a scripted batch, from both seeds, and counts the rounds either needs.

The batch runs with one sub-step per step (simulation_frequency = policy_frequency = 15: the kernels' dt), so that the
state planes before and after a step are the pre- and post-state of the sub-step its trace describes.  Per env and step:

  records   for every shielded lane (QP_ROWS != 0) evx = max(H1_VX, 1) (the committed v cos h), u0, v_min, v_max, g0 and the
            static parts of h0 / h3 are rebuilt from the planes and checked against the trace's QP_A, QP_H1, QP_H2 bit for bit;
  slots     which vehicle fills the leader (front-adjacent) slot is found as the one hypothesis -- nobody, the obstacle, or a
            vehicle of the env in its stepped (rank below mine: H1 record, decided acceleration, g.vx of the pose it
            commits) or unstepped form (H2 record, last safe acceleration) -- that gives the trace's QP_H0 (QP_H3) with the
            decisions the trace ends with: a lane for which no hypothesis fits fails the test;
  replay    the rounds, with the kernel's exit test and bound, from either seed.  The veto of a lane in the slow-LC bypass
            (the one decision that enters an acceleration) is taken from the trace's flags: it depends on the rear-adjacent
            slot, which the trace does not identify.

Both replays must end on the trace's QP_H0, QP_H3, QP_D and SAFE_ACC, bit for bit.  A wave of the kernel runs the rounds of
its 64 / G envs together and leaves when none of them changed: its count is the largest of its envs'.

The scenes, placed through the state planes before steps 3 and 9 (SCENES, env by env): a platoon closing in on a slow
vehicle (a chain of active followers), a stopped leader, a lane changer below the stopping speed (the slow-LC bypass), a
vehicle leaving its lane in front of a follower on the next lane (constrain_adj, h3 binding), and vehicles whose G_VX plane
the caller set to a negative value and to zero (g0 <= 0).  test_the_batch_holds_every_case counts them from the trace.
"""
import functools

import torch

import oracle_env
from marl_mass_amd import _cabi as abi

# (E envs, N vehicles) and the debug_flags of the device env: every group size the loop is compiled for, and the 16-lane
# groups the one way the library offers them (debug_flags bit 1)
SHAPES = {"E16_N8": (16, 8), "E10_N6": (10, 6), "E5_N12": (5, 12), "E5_N12_G16": (5, 12), "E5_N9": (5, 9), "E5_N9_G16": (5, 9),
          "E16_N4": (16, 4), "E32_N2": (32, 2)}
GPU_FLAGS = {"E5_N12_G16": 2, "E5_N9_G16": 2}
STEPS = 14
SCRIPT_AT = (3, 9)
TAPE_SEED = 53
P_ACT = torch.tensor([0.15, 0.4, 0.15, 0.2, 0.1])  # LEFT, IDLE, RIGHT, FASTER, SLOWER
BC0, BC1 = abi.LANE_ID[("b", "c", 0)], abi.LANE_ID[("b", "c", 1)]
DT, ETA, TAU = 1.0 / 15, 0.03125, 0.5
VEH_LENGTH, LC_MIN_ACC, LC_MAX_ACC, CBF_ACC_HI, PERCEPTION, ADJ_BUFFER, STOPPING_SPEED = 5.0, -12.5, 6.0, 6.0, 180.0, 2.0134, 1.6667
OBST_X, OBST_Y = 420.0, 4.0
# (env, vehicle, x, y, heading, lane, target lane, speed, target speed, G_VX or None, action or None)
SCENES = (
    # env 1: four vehicles 17.5 m apart on bc0 -- just inside the safe distance of 17.7 m at 15 m/s -- behind a slightly
    # slower one, all told to go FASTER: every follower's QP is active, none at its bound, each reads the one before
    (1, 0, 400.0, 0.0, 0.0, BC0, BC0, 14.9, 14.9, None, 3), (1, 1, 382.5, 0.0, 0.0, BC0, BC0, 15.0, 15.0, None, 3),
    (1, 2, 365.0, 0.0, 0.0, BC0, BC0, 15.0, 15.0, None, 3), (1, 3, 347.5, 0.0, 0.0, BC0, BC0, 15.0, 15.0, None, 3),
    (1, 4, 330.0, 0.0, 0.0, BC0, BC0, 15.0, 15.0, None, 3),
    # env 2: a leader that stands and brakes; its follower
    (2, 0, 350.0, 0.0, 0.0, BC0, BC0, 0.0, 0.0, None, 4), (2, 1, 338.0, 0.0, 0.0, BC0, BC0, 8.0, 8.0, None, 1),
    # env 3: a lane change commanded below the stopping speed, behind a slow leader
    (3, 0, 310.0, 0.0, 0.0, BC0, BC0, 1.0, 1.0, None, 1), (3, 1, 300.0, 0.0, 0.0, BC0, BC0, 1.0, 1.0, None, 2),
    # env 4 / 5: G_VX set by the caller: negative, zero
    (4, 0, 362.0, 0.0, 0.0, BC0, BC0, 10.0, 10.0, None, 1), (4, 1, 350.0, 0.0, 0.0, BC0, BC0, 15.0, 15.0, -0.5, 1),
    (5, 0, 362.0, 0.0, 0.0, BC0, BC0, 10.0, 10.0, None, 1), (5, 1, 350.0, 0.0, 0.0, BC0, BC0, 15.0, 15.0, 0.0, 1),
    # env 6: a vehicle of bc1 whose front-left corner hangs 0.1 m into bc0 (not heading there: front-adjacent, not a leader),
    # 19 m in front of a vehicle on bc0: inside the 19.7 m that constrain_adj asks for
    (6, 0, 359.0, 2.9, 0.0, BC1, BC1, 14.8, 14.8, None, 1), (6, 1, 340.0, 0.0, 0.0, BC0, BC0, 15.0, 15.0, None, 1),
)


def kw(nsub=1, seed=3141, **more):
    cfg = {"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}
    if nsub == 1:
        cfg.update(simulation_frequency=15, policy_frequency=15)
    d = dict(env_id="merge-multi-agent-v1", config=cfg, cbf_eta=ETA, cbf_tau=TAU, qp_solver="exact", obs_f64=True,
             auto_reset=True, seed=seed)
    d.update(more)
    return d


def actions(E, N, steps=STEPS, seed=TAPE_SEED):
    """The action tape; at the scripted steps the vehicles of the scenes take the action their scene names."""
    g = torch.Generator().manual_seed(seed)
    tape = [torch.multinomial(P_ACT, E * N, True, generator=g).view(E, N).int() for _ in range(steps)]
    for t in SCRIPT_AT:
        if t < steps:
            for sc in SCENES:
                if sc[0] < E and sc[1] < N and sc[10] is not None:
                    tape[t][sc[0], sc[1]] = sc[10]
    return tape


def script(env):
    """The caller's edit (state planes on the env's own device): the scenes the shape has envs and vehicles for."""
    F, B = abi.F, abi.B
    E, N = env.f64.shape[1], env.f64.shape[2]
    for e, v, x, y, h, lane, tlane, speed, tspeed, gvx, _ in SCENES:
        if e >= E or v >= N:
            continue
        env.f64[F["X"], e, v] = x
        env.f64[F["Y"], e, v] = y
        env.f64[F["HEADING"], e, v] = h
        env.f64[F["SPEED"], e, v] = speed
        env.f64[F["TARGET_SPEED"], e, v] = tspeed
        # the history records a vehicle driving like this would hold: x one and two sub-steps ago, its v cos h (heading 0: v)
        env.f64[F["H1_X"], e, v] = x
        env.f64[F["H1_VX"], e, v] = speed
        env.f64[F["H2_X"], e, v] = x - speed * DT
        env.f64[F["H2_VX"], e, v] = speed
        if gvx is not None:
            env.f64[F["G_VX"], e, v] = gvx
        env.u8[B["LANE"], e, v] = lane
        env.u8[B["TARGET_LANE"], e, v] = tlane
        env.u8[B["CRASHED"], e, v] = 0
        # (a turned vehicle's v cos h is the kernels' cosine, which the caller does not have: it drives its first sub-step
        # without a shield, like a vehicle just spawned, and holds the committed value from then on)
        env.u8[B["HIST_LEN"], e, v] = 2 if h == 0.0 else 1


def snap(env, step_result):
    obs, rew, done, info = step_result
    rec = {"f64": env.f64, "u8": env.u8, "env_i32": env.env_i32, "obs": obs, "reward": rew, "done": done}
    if env.trace is not None:
        rec["trace"] = env.trace
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


@functools.lru_cache(maxsize=None)
def oracle_tape(shape, nsub=1, steps=STEPS, scripted=True):
    """The oracle's run of a case, once: per step the record the GPU is compared with (trace included) and the planes before it."""
    E, N = SHAPES[shape]
    oracle_env.set_math_mode(1)  # include/mm_math.h on both sides: bit-for-bit comparison
    try:
        env = oracle_env.OracleEnv(E, N, trace=True, **kw(nsub))
        env.reset()
        tape = []
        for t, a in enumerate(actions(E, N, steps)):
            if scripted and t in SCRIPT_AT:
                script(env)
            pre = {"u8": env.u8.clone(), "f64": env.f64.clone()}
            tape.append({"rec": snap(env, env.step(a)), "pre": pre, "act": a})
        return tape
    finally:
        oracle_env.set_math_mode(0)


# ---- the replay -------------------------------------------------------------------------------------------------------
def bits(x):
    return torch.tensor(float(x), dtype=torch.float64).view(torch.int64).item()


def eq(a, b):
    return bits(a) == bits(b) or (a != a and b != b)


def slot_gu(vx, acc, g):
    u = vx + acc * DT
    u = u if u > 0 else 0.0
    return (g * DT) * u


def records(st, e):
    """The lanes of env e in the sub-step of tape entry st, or None where the planes after the step are not the sub-step's
    post-state (the episode ended there and the env was respawned)."""
    F, B, T = abi.F, abi.B, abi.T
    pre, post, tr = st["pre"], st["rec"]["f64"], st["rec"]["trace"][0]
    if bool(st["rec"]["done"][e]):
        return None
    N = tr.shape[2]
    f = lambda p, i: float(pre["f64"][F[p], e, i])  # noqa: E731
    t_ = lambda p, i: float(tr[T[p], e, i])  # noqa: E731
    live = [int(pre["u8"][B["KIND"], e, i]) != 0 and not (t_("X", i) != t_("X", i)) for i in range(N)]
    lanes = []
    for i in range(N):
        if not live[i]:
            lanes.append(None)
            continue
        x = f("X", i)
        rank = sum(1 for j in range(N) if j != i and live[j] and (f("X", j) > x or (f("X", j) == x and j < i)))
        shielded = t_("QP_ROWS", i) != 0
        L = {"i": i, "x": x, "y": f("Y", i), "rank": rank, "shielded": shielded, "act_acc": t_("ACT_ACC", i),
             "h1x": f("H1_X", i), "h1vx": f("H1_VX", i), "h2x": f("H2_X", i), "h2vx": f("H2_VX", i),
             "sacc": f("SAFE_ACC", i), "g_pre": f("G_VX", i), "g_post": float(post[F["G_VX"], e, i]),
             "final_acc": t_("SAFE_ACC", i) if shielded else t_("ACT_ACC", i)}
        if shielded:
            v = f("SPEED", i)
            hl = int(st["act"][e, i])
            v_min = v + LC_MIN_ACC * DT
            v_min = v_min if v_min > 0 else 0.0
            v_max = v + LC_MAX_ACC * DT
            evx = L["h1vx"] if L["h1vx"] > 1 else 1.0
            u0 = evx + L["act_acc"] * DT
            u0 = u0 if u0 > 0 else 0.0
            buffer = (CBF_ACC_HI + 0.1) * DT * TAU
            sd0 = evx * TAU + VEH_LENGTH + buffer
            L.update(v=v, evx=evx, u0=u0, g0=L["g_pre"] * DT, h1=v_max - u0, h2=-v_min + u0, q_lon=-VEH_LENGTH - sd0,
                     q_lona=-VEH_LENGTH - sd0 - ADJ_BUFFER, cadj=t_("QP_ROWS", i) == 4, slow_lc=hl in (0, 2) and v < STOPPING_SPEED,
                     veto=(int(t_("FLAGS", i)) & abi.FLAG_IS_LC_SAFE) == 0,
                     want={k: t_(k, i) for k in ("QP_H0", "QP_H3", "QP_D", "SAFE_ACC")})
            assert eq(L["g0"], t_("QP_A", i)) and eq(L["h1"], t_("QP_H1", i)) and eq(L["h2"], t_("QP_H2", i)), (e, i, "static rows")
        lanes.append(L)
    for L in lanes:
        if L is not None and L["shielded"]:
            L["ol"] = find_slot(L, lanes, L["q_lon"], L["want"]["QP_H0"], (e, L["i"], "leader"))
            L["oa"] = find_slot(L, lanes, L["q_lona"], L["want"]["QP_H3"], (e, L["i"], "front-adjacent")) if L["cadj"] else None
    return lanes


def row(L, q, x_o, gu):
    px = x_o - L["x"]
    base = px + (ETA - 1) * px + ETA * q
    return base + (-(L["g0"] * L["u0"]) + gu)


def find_slot(L, lanes, q, want, where):
    """(x of the slot's record, its g*u product or None if it follows the owner's decision, owner)"""
    hyp = [(L["x"] + PERCEPTION + 1, 0.0, None), (OBST_X, 0.0, None)]
    for O in lanes:
        if O is None or O is L:
            continue
        if O["rank"] < L["rank"]:
            hyp.append((O["h1x"], None, O))  # stepped before me: its post-step record under its decision
        else:
            hyp.append((O["h2x"], slot_gu(O["h2vx"], O["sacc"], O["g_pre"]), None))
    fits = []
    for x_o, gu, O in hyp:
        g = gu if O is None else slot_gu(O["h1vx"], O["final_acc"], O["g_post"])
        if eq(row(L, q, x_o, g), want):
            fits.append((x_o, gu, O))
    assert fits, where
    assert len({(bits(x_o), O["i"] if O else -1) for x_o, gu, O in fits}) == 1, (where, "ambiguous")
    return fits[0]


def replay(lanes, prior):
    """The rounds of one env: (rounds run, lanes)."""
    N = len(lanes)
    on = [L for L in lanes if L is not None]
    for L in on:
        L["acc"] = (((L["u0"] - L["evx"]) / DT) if prior else 0.0) if L["shielded"] else L["act_acc"]
    rounds = 0
    for rnd in range(N + 1):
        rounds += 1
        gu_cur = {L["i"]: slot_gu(L["h1vx"], L["acc"], L["g_post"]) for L in on}
        changed = False
        nxt = {}
        for L in on:
            if not L["shielded"]:
                nxt[L["i"]] = L["act_acc"]
                continue
            x_ol, gu, O = L["ol"]
            h0 = row(L, L["q_lon"], x_ol, gu if O is None else gu_cur[O["i"]])
            h3 = float("nan")
            if L["cadj"]:
                x_oa, gu, O = L["oa"]
                h3 = row(L, L["q_lona"], x_oa, gu if O is None else gu_cur[O["i"]])
            hc = h3 if (L["cadj"] and h3 < h0) else h0  # qp_exact
            if L["g0"] > 0:
                d = min(0.0, hc / L["g0"])
            elif L["g0"] < 0:
                d = max(0.0, hc / L["g0"])
            else:
                d = 0.0
            d = min(max(d, -L["h2"]), L["h1"])
            us0 = L["u0"] + d
            if L["slow_lc"] and not L["veto"]:
                us0 = L["u0"]
            nxt[L["i"]] = (us0 - L["evx"]) / DT
            L["got"] = {"QP_H0": h0, "QP_H3": h3, "QP_D": d}
        for L in on:
            changed = changed or bits(nxt[L["i"]]) != bits(L["acc"])
            L["acc"] = nxt[L["i"]]
        if not changed:
            break
    for L in on:
        if L["shielded"]:
            L["got"]["SAFE_ACC"] = L["acc"]
    return rounds


@functools.lru_cache(maxsize=None)
def replayed(shape="E16_N8"):
    """Every (step, env) of the tape whose sub-step can be replayed: rounds from either seed and the cases it holds."""
    out = []
    for t, st in enumerate(oracle_tape(shape)):
        for e in range(SHAPES[shape][0]):
            lanes = records(st, e)
            if lanes is None or not any(L is not None and L["shielded"] for L in lanes):
                continue
            got = {}
            for prior in (False, True):
                r = replay(lanes, prior)
                got[prior] = (r, {L["i"]: dict(L["got"]) for L in lanes if L is not None and L["shielded"]})
            sh = [L for L in lanes if L is not None and L["shielded"]]
            active = {L["i"] for L in sh if L["want"]["QP_D"] != 0.0}
            chain = 0  # active followers in a row, each reading the decision of the one before
            for L in sh:
                n, cur = 0, L
                while cur is not None and cur["shielded"] and cur["i"] in active and cur["ol"][2] is not None:
                    n, cur = n + 1, cur["ol"][2]
                chain = max(chain, n)
            out.append({"t": t, "e": e, "lanes": lanes, "got": got, "active": len(active), "chain": chain,
                        "moved": any(L["want"]["SAFE_ACC"] != 0.0 for L in sh),
                        "slow_lc": sum(1 for L in sh if L["slow_lc"]),
                        "h3_binds": sum(1 for L in sh if L["cadj"] and L["i"] in active and L["want"]["QP_H3"] < L["want"]["QP_H0"]),
                        "stopped_leader": sum(1 for L in sh if L["ol"][2] is not None and L["ol"][2]["final_acc"] < 0 and
                                              L["ol"][2]["h1vx"] + L["ol"][2]["final_acc"] * DT <= 0),
                        "g0_neg": sum(1 for L in sh if L["g0"] < 0), "g0_zero": sum(1 for L in sh if L["g0"] == 0)})
    return out


def test_both_seeds_end_on_the_oracles_answer():
    cases = replayed()
    assert len(cases) >= 50
    for c in cases:
        for prior in (False, True):
            for L in c["lanes"]:
                if L is None or not L["shielded"]:
                    continue
                for k, w in L["want"].items():
                    assert eq(c["got"][prior][1][L["i"]][k], w), (c["t"], c["e"], L["i"], k, "prior" if prior else "zero")
        # the kernel's bound holds from either seed.  (The prior is not always the shorter way: a follower whose QP is inactive
        # under its leader's final decision can be active under the leader's SEED, and then needs a round to come back.)
        N = len(c["lanes"])
        assert max(c["got"][True][0], c["got"][False][0]) <= N + 1, (c["t"], c["e"], c["got"][False][0], c["got"][True][0])
    n0, n1 = sum(c["got"][False][0] for c in cases), sum(c["got"][True][0] for c in cases)
    worse = [(c["t"], c["e"], c["got"][False][0], c["got"][True][0]) for c in cases if c["got"][True][0] > c["got"][False][0]]
    # (printed, not bounded: how many envs take longer from the prior is a property of the batch, not of the kernel -- the answers
    # are bit-equal either way, which is what is asserted above)
    print("env sub-steps %d: rounds from 0.0 %d, from the prior %d; longer from the prior: %s" % (len(cases), n0, n1, worse))


def test_an_env_without_an_active_qp_needs_one_round_instead_of_two():
    quiet = [c for c in replayed() if c["active"] == 0]
    assert quiet
    for c in quiet:
        assert c["got"][True][0] == 1, (c["t"], c["e"])           # the seed is the answer: the first round confirms it
        assert c["got"][False][0] == (2 if c["moved"] else 1), (c["t"], c["e"])  # from 0.0: one round to get there, one to confirm
    assert sum(1 for c in quiet if c["moved"]) >= 10


def test_the_batch_holds_every_case():
    cases = replayed()
    tot = {k: sum(int(c[k]) for c in cases) for k in ("slow_lc", "h3_binds", "stopped_leader", "g0_neg", "g0_zero")}
    longest = max(cases, key=lambda c: c["chain"])
    print(tot, "longest chain", longest["chain"], "rounds from 0.0 / from the prior", longest["got"][False][0], longest["got"][True][0])
    assert longest["chain"] >= 3           # a platoon with at least three active followers in a row
    # Convention (the kernel's comment at the seed counts the same way): `chain` = L counts the active followers only, not the
    # inactive vehicle in front of them, and a round count includes the confirming round.  From 0.0 the front vehicle (told to
    # accelerate) moves in round 0 and the k-th follower in round k: L + 2 rounds; from the prior the front vehicle starts
    # final and the k-th follower moves in round k - 1: L + 1.
    assert (longest["got"][False][0], longest["got"][True][0]) == (longest["chain"] + 2, longest["chain"] + 1)
    assert tot["slow_lc"] >= 1             # hl 0 / 2 below the stopping speed
    assert tot["h3_binds"] >= 1            # constrain_adj, and the front-adjacent row is the binding one
    assert tot["stopped_leader"] >= 1      # a stepped leader whose u = max(0, vx + acc dt) is clipped at 0
    assert tot["g0_neg"] >= 1 and tot["g0_zero"] >= 1  # g0 <= 0: the other branches of the exact QP


# ---- the sine lane from one sub-step to the next ----------------------------------------------------------------------------
# What a step kernel could carry from predict's closest_lane to the next sub-step's steering_control is the sine of kb0's frame
# at the committed x (MM_SINE_CARRY).  Placed vehicles drive through the cases in which such a value is there,
# is missing, or belongs to the other candidate; tests/test_rounds_prior_gpu.py steps them against this tape.
import math  # noqa: E402

RAMP_STEPS = 12
AB0, JK0, KB0 = abi.LANE_ID[("a", "b", 0)], abi.LANE_ID[("j", "k", 0)], abi.LANE_ID[("k", "b", 0)]


def _kb0(x):
    """A pose on the centre line of kb0 (amplitude 3.25, pulsation 2 pi / 200, phase pi / 2 from x = 220)."""
    ph = math.pi / 100.0 * (x - 220.0) + math.pi / 2
    return 7.25 + 3.25 * math.sin(ph), math.atan(3.25 * math.pi / 100.0 * math.cos(ph))


def ramp_spawn(E, N=8):
    """[E, N] x, y, heading, speed and the action of every step (1 idle, 0 lane change, 3 / 4 faster / slower)."""
    rows = [(207.0, 10.5, 0.0, 1),           # jk0: its lane becomes kb0 at x = 220, in the middle of a step
            (240.0,) + _kb0(240.0) + (1,),   # kb0, sub-step after sub-step
            (226.0, 0.0, 0.0, 1),            # exactly on ab0 beside the ramp: closest_lane's early-out, no sine at all
            (331.0, 4.0, 0.0, 0),            # bc1, asks for bc0 at every step ...
            (333.0, 0.0, 0.0, 1),            # ... where this one drives beside it: vetoed, candidate B is the one committed
            (270.0,) + _kb0(270.0) + (3,),   # kb0, accelerating
            (172.0, 10.5, 0.0, 3), (150.0, 0.0, 0.0, 4)][:N]
    t = torch.tensor([r[:3] for r in rows], dtype=torch.float64)
    x = t[None, :, 0].repeat(E, 1) + 0.29 * torch.arange(E, dtype=torch.float64)[:, None] * torch.tensor([1.0, 1, 0, 0, 0, 1, 1, 1][:N])[None]
    y, h = t[None, :, 1].repeat(E, 1), t[None, :, 2].repeat(E, 1)
    # (the kb0 vehicles of the shifted envs start beside the centre line by up to 0.4 m and steer back: more of the frame's range)
    act = torch.tensor([r[3] for r in rows], dtype=torch.int32)[None].repeat(E, 1)
    return x.numpy(), y.numpy(), h.numpy(), torch.full((E, N), 25.0, dtype=torch.float64).numpy(), act


def ramp_run(make, E=16, N=8, **more):
    env = make(E, N, **kw(3, seed=99, **more))
    x, y, h, v, act = ramp_spawn(E, N)
    env.set_kinematics(x, y, h, v)
    a = act.to(env.device)
    tape = [snap(env, env.step(a)) for _ in range(RAMP_STEPS)]
    if hasattr(env, "poll_errors"):
        env.poll_errors()
    env.close()
    return tape


@functools.lru_cache(maxsize=None)
def ramp_oracle_tape():
    oracle_env.set_math_mode(1)
    try:
        return ramp_run(oracle_env.OracleEnv, trace=True)
    finally:
        oracle_env.set_math_mode(0)


def test_the_ramp_tape_holds_every_sub_step_case():
    T = abi.T
    tr = torch.stack([r["trace"] for r in ramp_oracle_tape()])  # [steps, 3, planes, E, N]
    x, y, h = tr[:, :, T["X"]], tr[:, :, T["Y"]], tr[:, :, T["HEADING"]]
    lane, tl = tr[:, :, T["LANE"]], tr[:, :, T["TARGET_LANE"]]
    ran = ~torch.isnan(x)
    nxt = ran[:, 1:] & ran[:, :-1]  # a sub-step and the one before it, in one step (one launch of the fused kernels)
    # on kb0 and steering along kb0 in the next sub-step of the same step: the frame's sine at the committed x is wanted again
    assert int((nxt & (lane[:, :-1] == KB0) & (tl[:, 1:] == KB0)).sum()) > 100
    # jk0 -> kb0 between two sub-steps of one step, the target already kb0
    assert bool((nxt & (lane[:, :-1] == JK0) & (lane[:, 1:] == KB0) & (tl[:, 1:] == KB0)).any())
    # exactly on ab0 beside the ramp, sub-step after sub-step: closest_lane leaves before the frame
    assert bool((nxt & (lane[:, 1:] == AB0) & (y[:, 1:] == 0.0) & (h[:, 1:] == 0.0) & (x[:, 1:] > 220.0) & (x[:, 1:] < 320.0)).any())
    # a veto that committed candidate B (the integrated steering is not the nominal one), followed by a sub-step of the same step
    veto = ran & (tr[:, :, T["QP_ROWS"]] > 0) & (tr[:, :, T["SAFE_STEER"]] != tr[:, :, T["ACT_STEER"]])
    assert bool((veto[:, :-1] & ran[:, 1:]).any())

