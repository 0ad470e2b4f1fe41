"""The scripted batch of tests/test_partner_exchange_gpu.py, and what it must contain (CPU, oracle only).

The partner exchanges of step_kernel (the DPP helper every power-of-two group kernel shares, the sweep rank, the collision
pre-check) decide nothing in an env whose vehicles drive far apart, so a parity test over a fresh batch would pass whatever
they returned.  The batch is therefore scripted through the caller's state planes: before steps 2 and 8 of its 12 steps (the
shields are on by then, and until then no wave holds a near pair) the caller places vehicles of the first envs (as many of
the scenes as the shape has envs for; the first three fit every shape)

  env 0  two vehicles with EQUAL x side by side on bc0 / bc1: a rank tie (decided by the creation index) that is also a near
         pair (4 m apart, inside the 5 m pre-check) whose boxes do not touch;
  env 1  two vehicles on bc0 whose boxes overlap: they collide in the first sub-step, which ends the episode there -- the
         rank formed for the next sub-step is never read;
  env 2  a vehicle on bc1 driving into the obstacle at its end;
  env 3  a near pair on bc0 / bc1 with different x that does not touch;
  env 4  a vehicle on bc1 already inside the obstacle's box.

The rest of the batch drives on from the reset (or the respawn): waves without a near pair.  The cases are counted here from
the oracle's per-sub-step trace alone (math mode 1), so that the GPU test cannot pass on a batch that lost them:

  near       (pair, sub-step): both live, centres within 5 m after the commit, no crash between the two
  collide    vehicles whose crashed flag rises in a sub-step with a live partner within 5 m
  obstacle   vehicles whose crashed flag rises within 5 m of the obstacle
  tie        (pair, sub-step): equal x at the START of the sub-step; "carried": in a sub-step after the first of its step,
             where the fused kernels take the rank from the previous sub-step's collision loop
  early      envs whose episode ends in sub-step 0 or 1 of a step
  quiet      (wave, sub-step): a wave of the kernel (64 / G envs) with live vehicles and no near pair
"""
import functools

import torch

import oracle_env
from marl_mass_amd import _cabi as abi

# (E envs, N vehicles): 8-, 4- and 2-lane groups with and without an absent lane, and the 6-lane rotation layout.  An env holds at
# most 12 vehicles (6 + 6 spawn slots), and 9..12 of them step in the 12-lane rotation layout, so the 16-lane groups -- the
# row_ror:8 and row_mirror exchanges -- are reached the one way the library offers: debug_flags bit 1 (power-of-two groups
# only), with a full complement of 12 vehicles and with 9, the fewest a 16-lane group is used for.
SHAPES = {"E9_N8": (9, 8), "E9_N7": (9, 7), "E5_N4": (5, 4), "E5_N3": (5, 3), "E3_N2": (3, 2), "E5_N12_G16": (5, 12),
          "E5_N9_G16": (5, 9), "E11_N6": (11, 6)}
GPU_FLAGS = {"E5_N12_G16": 2, "E5_N9_G16": 2}  # debug_flags of the device env (the oracle has one form only)
SHIELDS = {"mass": "cbf-cav", "hss": "cbf-avs_cint"}
STEPS = 12
SCRIPT_AT = (2, 8)
TAPE_SEED = 47
P_ACT = torch.tensor([0.15, 0.4, 0.15, 0.2, 0.1])  # LEFT, IDLE, RIGHT, FASTER, SLOWER
OBST_X, OBST_Y = 420.0, 4.0
BC0, BC1 = abi.LANE_ID[("b", "c", 0)], abi.LANE_ID[("b", "c", 1)]
# (env, vehicle, x, y, lane, speed): the scenes above; vehicles 0 and 1 exist in every shape
SCENES = ((0, 0, 350.0, 0.0, BC0, 20.0), (0, 1, 350.0, 4.0, BC1, 20.0),
          (1, 0, 340.0, 0.0, BC0, 22.0), (1, 1, 343.5, 0.0, BC0, 18.0),
          (2, 0, 415.25, 4.0, BC1, 20.0),
          (3, 0, 360.0, 0.0, BC0, 21.0), (3, 1, 361.5, 4.0, BC1, 21.0),
          (4, 1, 417.5, 4.0, BC1, 15.0))


def group(shape):
    """Lanes per env in the kernel's layout: power-of-two groups, or the 6-lane rotation layout (N = 5..6)."""
    N = SHAPES[shape][1]
    if N in (5, 6) and not GPU_FLAGS.get(shape):
        return 6
    return 1 << max(N - 1, 1).bit_length()


def kw(shield, seed=2718, **more):
    d = dict(env_id="merge-multi-agent-v1", config={"safety_guarantee": SHIELDS[shield], "HEADWAY_TIME": 0.5},
             cbf_eta=0.03125, cbf_tau=0.5, qp_solver="exact", obs_f64=True, auto_reset=True, seed=seed)
    d.update(more)
    return d


def actions(E, N, steps=STEPS, seed=TAPE_SEED):
    g = torch.Generator().manual_seed(seed)
    return [torch.multinomial(P_ACT, E * N, True, generator=g).view(E, N).int() for _ in range(steps)]


def script(env):
    """The caller's edit (state planes on the env's own device): the scenes the shape has envs for."""
    F, B = abi.F, abi.B
    E = env.f64.shape[1]
    for e, v, x, y, lane, speed in SCENES:
        if e >= E:
            continue
        env.f64[F["X"], e, v] = x
        env.f64[F["Y"], e, v] = y
        env.f64[F["HEADING"], e, v] = 0.0
        env.f64[F["SPEED"], e, v] = speed
        env.f64[F["TARGET_SPEED"], e, v] = speed
        env.u8[B["LANE"], e, v] = lane
        env.u8[B["TARGET_LANE"], e, v] = lane
        env.u8[B["CRASHED"], e, v] = 0


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


@functools.lru_cache(maxsize=None)
def oracle_tape(shape, shield):
    """The oracle's run of a case, once: per step the record the GPU is compared with, the state before it and the trace."""
    E, N = SHAPES[shape]
    oracle_env.set_math_mode(1)  # include/mm_math.h on both sides: bit-for-bit comparison
    try:
        env = oracle_env.OracleEnv(E, N, trace=True, **kw(shield))
        env.reset()
        tape = []
        for t, a in enumerate(actions(E, N)):
            if t in SCRIPT_AT:
                script(env)
            pre = {"u8": env.u8.clone(), "f64": env.f64[:2].clone()}
            rec = snap(env, env.step(a))
            tape.append({"rec": rec, "pre": pre, "trace": env.trace.clone()})
        return tape
    finally:
        oracle_env.set_math_mode(0)


def count_cases(tape, shape):
    T, B, F = abi.T, abi.B, abi.F
    N, per_wave = SHAPES[shape][1], 64 // group(shape)
    n = {"near": 0, "collide": 0, "obstacle": 0, "tie": 0, "tie_carried": 0, "early": 0, "quiet": 0, "busy": 0}
    for st in tape:
        tr, pre = st["trace"], st["pre"]
        nsub, E = tr.shape[0], tr.shape[2]
        present = pre["u8"][B["KIND"]] != 0                                   # [E, N]
        x0, crashed0 = pre["f64"][F["X"]].double(), pre["u8"][B["CRASHED"]] != 0
        for k in range(nsub):
            x, y = tr[k, T["X"]], tr[k, T["Y"]]
            live = present & ~torch.isnan(x)                                  # the env was still active in sub-step k
            crashed = tr[k, T["CRASHED"]].nan_to_num() != 0
            xs = x0 if k == 0 else tr[k - 1, T["X"]]                          # x at the start of sub-step k
            pair = live[:, :, None] & live[:, None, :] & torch.triu(torch.ones(N, N, dtype=torch.bool), 1)[None]
            ties = int((pair & (xs[:, :, None] == xs[:, None, :])).sum())
            n["tie"] += ties
            n["tie_carried"] += ties if k > 0 else 0
            d2 = (x[:, :, None] - x[:, None, :]) ** 2 + (y[:, :, None] - y[:, None, :]) ** 2
            near = pair & (d2.sqrt() <= 5.0)
            rose = live & crashed & ~crashed0
            touching = near & (rose[:, :, None] | rose[:, None, :])
            n["near"] += int((near & ~touching).sum())
            n["collide"] += int((rose & (touching.any(2) | touching.any(1))).sum())
            n["obstacle"] += int((rose & (((x - OBST_X) ** 2 + (y - OBST_Y) ** 2).sqrt() <= 5.0) & ~(touching.any(2) | touching.any(1))).sum())
            if k + 1 < nsub:
                gone = live.any(1) & torch.isnan(tr[k + 1, T["X"]]).all(1)   # the episode ended with sub-step k < nsub - 1
                n["early"] += int(gone.sum())
            for w in range(0, E, per_wave):
                if bool(live[w:w + per_wave].any()):
                    n["busy" if bool(near[w:w + per_wave].any()) else "quiet"] += 1
            crashed0 = crashed
    return n


@functools.lru_cache(maxsize=None)
def totals():
    return {(shape, shield): count_cases(oracle_tape(shape, shield), shape) for shield in SHIELDS for shape in SHAPES}


def test_every_tape_contains_every_case():
    per = totals()
    for key in sorted(per):
        print(key, per[key])
    for key, c in per.items():
        assert c["near"] >= 1, (key, c)         # side by side within 5 m, boxes apart
        assert c["collide"] >= 2, (key, c)      # both vehicles of a colliding pair
        assert c["obstacle"] >= 1, (key, c)
        assert c["tie"] >= 1, (key, c)
        assert c["tie_carried"] >= 1, (key, c)  # ... in a sub-step whose rank the fused kernels carry over
        assert c["early"] >= 1, (key, c)        # an episode that ends in sub-step 0 or 1
        assert c["quiet"] >= 1, (key, c)        # a wave without a near pair
        assert c["busy"] >= 1, (key, c)         # ... and a wave with one


def test_a_whole_wave_stays_quiet_beside_a_busy_one():
    """9 x 8 is two waves: the scenes live in the first, the ninth env alone in the second never holds a near pair."""
    for shield in SHIELDS:
        for st in oracle_tape("E9_N8", shield):
            tr = st["trace"]
            x, y = tr[:, abi.T["X"], 8], tr[:, abi.T["Y"], 8]  # [nsub, N]
            d2 = (x[:, :, None] - x[:, None, :]) ** 2 + (y[:, :, None] - y[:, None, :]) ** 2
            off = ~torch.eye(8, dtype=torch.bool)[None]
            assert not bool(((d2.sqrt() <= 5.0) & off).any()), shield
