"""The sine lane's frame in the fused exact-mode step kernels: mmm_atan_small and one mmm_sincos in closest_lane (the 2- / 4- /
8-lane kernels), next_lane from the pose code in the epilogue (every shielded kernel).

Nothing about the results may change, so placed vehicles are driven over every case of the frame -- jk0 -> kb0 (the target
follows the road onto kb0 at x = 217.5, the vehicle at x = 220), kb0 -> bc1 at x = 320, a vehicle exactly on ab0 with heading
0 beside the ramp (closest_lane's early-out skips the frame), a vetoed lane change on bc1 (candidate B, steered to the
current lane, is the one committed) -- and state, observation, reward, done and the info dict are compared with the oracle
bit for bit, in the production and the trace instantiation, in the parallel and the literal form of the sweep.  E = 10,
N = 6 is the 6-lane rotation layout (several groups and idle tail lanes in a wave), which keeps the general forms."""
import functools

import numpy as np
import pytest
import torch

import oracle_env
from golden_util import env_kwargs
from marl_mass_amd import VecMergeEnv, _cabi as abi

AB0, BC0, BC1, CD0, JK0, KB0 = range(6)
STEPS = 40
SHAPES = {"E16_N8": (16, 8), "E10_N6": (10, 6)}  # the second: 6-lane rotation layout, several groups and idle tail lanes in a wave


def _kb0(x):
    """A pose on the centre line of kb0 (merge_env_v1.py:222-248: amplitude 3.25, pulsation 2 pi / 200, phase pi / 2)."""
    ph = np.pi / 100.0 * (x - 220.0) + np.pi / 2
    return 7.25 + 3.25 * np.sin(ph), np.arctan(3.25 * np.pi / 100.0 * np.cos(ph))


def _spawn(E, N):
    """[E, N] x, y, heading, speed and the action of every step."""
    y240, h240 = _kb0(240.0)
    y290, h290 = _kb0(290.0)
    rows = [  # x, y, heading, action (1 idle, 0 / 2 lane change, 3 / 4 faster / slower)
        (203.0, 10.5, 0.0, 1),   # jk0: crosses x = 217.5 (target -> kb0) and x = 220 (lane -> kb0), later kb0 -> bc1
        (240.0, y240, h240, 1),  # kb0
        (290.0, y290, h290, 1),  # kb0: reaches bc1 within a second
        (226.0, 0.0, 0.0, 1),    # exactly on ab0, heading 0, beside the ramp: closest_lane's early-out (bd == 0)
        (331.0, 4.0, 0.0, 0),    # bc1, asks for bc0 at every step ...
        (333.0, 0.0, 0.0, 1),    # ... where this one drives beside it: the shield vetoes, candidate B is committed
        (172.0, 10.5, 0.0, 3),   # jk0, further back
        (150.0, 0.0, 0.0, 4),    # ab0, further back
    ][:N]
    r = np.array([row[:3] for row in rows])
    x = np.repeat(r[None, :, 0], E, 0)
    # every env at its own phase of the ramp (0.37 m apart); the bc0 / bc1 pair and the ab0 vehicle keep their places
    shift = 0.37 * np.arange(E)[:, None] * np.array([1, 0, 0, 0, 0, 0, 1, 1][:N])[None, :]
    x = x + shift
    y, h = np.repeat(r[None, :, 1], E, 0), np.repeat(r[None, :, 2], E, 0)
    act = np.repeat(np.array([row[3] for row in rows], dtype=np.int32)[None], E, 0)
    return x, y, h, np.full((E, N), 25.0), act


def _kw(trace, debug_flags=0):
    kw = env_kwargs({"shield": "cbf-cav", "headway_time": 0.5, "env_id": "merge-multi-agent-v1", "eta": 0.03125})  # exact QP, f64 obs
    kw.update(seed=99, auto_reset=True, trace=trace, debug_flags=debug_flags)
    return kw


def _run(make, E, N, trace, debug_flags=0, keep_trace=False):
    """40 steps from the placed spawn -> per step (state f64, state u8, obs, reward, done, info dict[, trace]) on the CPU."""
    env = make(E, N, **_kw(trace, debug_flags))
    x, y, h, v, act = _spawn(E, N)
    env.set_kinematics(x, y, h, v)
    a = torch.as_tensor(act).to(env.device)
    tape = []
    for t in range(STEPS):
        obs, rew, done, info = env.step(a)
        rec = {"f64": env.f64, "u8": env.u8, "obs": obs, "reward": rew, "done": done}
        rec.update({"info." + k: w for k, w in info.items()})
        if keep_trace:
            rec["trace"] = env.trace
        tape.append({k: w.detach().cpu().clone() for k, w in rec.items()})
    if hasattr(env, "poll_errors"):
        env.poll_errors()
    env.close()
    return tape


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    """The oracle's run of a shape, once for every test (its results do not depend on the trace planes being written)."""
    E, N = SHAPES[shape]
    oracle_env.set_math_mode(1)  # include/mm_math.h on both sides
    try:
        return _run(oracle_env.OracleEnv, E, N, True, keep_trace=True)
    finally:
        oracle_env.set_math_mode(0)


def _same(a, b):
    if a.is_floating_point():
        a, b = a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)
    return torch.equal(a, b)


def test_scenario_covers_every_case():
    """(CPU) the oracle's own trace of the placed scenario: every case occurs, in both shapes."""
    T = abi.T
    for shape in SHAPES:
        tr = torch.stack([r["trace"] for r in _oracle(shape)]).numpy()  # [steps, 3, planes, E, N]
        tr = tr.reshape(-1, *tr.shape[2:])                                     # sub-steps in order
        x, y, h = tr[:, T["X"]], tr[:, T["Y"]], tr[:, T["HEADING"]]
        lane, tl = tr[:, T["LANE"]], tr[:, T["TARGET_LANE"]]
        ran = ~np.isnan(x)
        # the target lane is kb0 while the vehicle is still on jk0 before x = 220; then the vehicle is on kb0 itself
        assert (ran & (lane == JK0) & (tl == KB0) & (x > 217.5) & (x < 220.0)).any(), shape
        assert ((lane[:-1] == JK0) & (lane[1:] == KB0) & ran[1:]).any(), shape
        assert ((lane[:-1] == KB0) & (lane[1:] == BC1) & ran[1:]).any(), shape
        assert (ran & (lane == AB0) & (y == 0.0) & (h == 0.0) & (x > 220.0) & (x < 320.0)).any(), shape
        # a veto on bc1 that committed candidate B: the integrated steering is not the nominal one
        veto = ran & (lane == BC1) & (tr[:, T["SAFE_STEER"]] != tr[:, T["ACT_STEER"]]) & (tr[:, T["QP_ROWS"]] > 0)
        assert veto.any(), shape
        # ... and vehicles steering along kb0 one sub-step after another
        assert (ran[1:] & (lane[:-1] == KB0) & (tl[1:] == KB0)).sum() > 100, shape


@pytest.mark.gpu
@pytest.mark.parametrize("debug_flags", [0, 1], ids=["parallel", "literal"])
@pytest.mark.parametrize("trace", [False, True], ids=["production", "trace"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sine_frame_against_oracle(shape, trace, debug_flags):
    E, N = SHAPES[shape]
    want = [{k: w for k, w in r.items() if k != "trace"} for r in _oracle(shape)]
    got = _run(lambda E, N, **kw: VecMergeEnv(E, N, device="cuda:0", **kw), E, N, trace, debug_flags)
    for t, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w)
        for k in sorted(w):
            assert _same(g[k], w[k]), (shape, trace, debug_flags, t, k)
