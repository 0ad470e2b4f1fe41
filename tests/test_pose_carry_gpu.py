"""Derived pose values carried from launch to launch (PoseBuf / kCarry in step_kernel), in the fused exact-mode CAV-only
kernels of the 2- / 4- / 8-lane groups.

Nothing about the results may change:

* parity -- 120 auto-resetting steps (duration 20 s x 5 Hz = 100 steps, so every env re-spawns) against the CPU oracle bit for
  bit, MASS and HSS, at 9 x 8 (two waves, the second partly empty), 5 x 4, and 5 x 5 (the 6-lane rotation layout, which does
  not carry);
* staleness -- a handle whose carried planes no longer describe the caller's state (the caller edited it, reset a subset of
  envs, loaded a checkpoint; or the handle is fresh) steps exactly like a fresh handle on that state;
* a captured graph of 4 steps, replayed twice, equals the eager run.
"""
import functools

import pytest
import torch

import oracle_env
from marl_mass_amd import VecMergeEnv, _cabi as abi

SHAPES = {"E9_N8": (9, 8), "E5_N4": (5, 4), "E5_N5": (5, 5)}
SHIELDS = {"mass": "cbf-cav", "hss": "cbf-av"}
STEPS = 120
P_ACT = torch.tensor([0.15, 0.5, 0.15, 0.1, 0.1])


def _kw(shield, seed=4242):
    return dict(env_id="merge-multi-agent-v1", config={"safety_guarantee": SHIELDS[shield], "HEADWAY_TIME": 0.5},
                cbf_eta=0.03125, cbf_tau=0.5, qp_solver="exact", obs_f64=True, auto_reset=True, seed=seed)


def _actions(E, N, steps, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.multinomial(P_ACT, E * N, True, generator=g).view(E, N).int() for _ in range(steps)]


def _snap(env, step_result):
    obs, rew, done, info = step_result
    rec = {"f64": env.f64, "u8": env.u8, "env_i32": env.env_i32, "obs": obs, "reward": rew, "done": done}
    rec.update({"info." + k: w for k, w in info.items()})
    return {k: w.detach().cpu().clone() for k, w in rec.items()}


def _same(a, b):
    if a.is_floating_point():
        return torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)) and torch.equal(a.isnan(), b.isnan())
    return torch.equal(a, b)


def _assert_same(got, want, where):
    assert set(got) == set(want), where
    for k in sorted(want):
        assert _same(got[k], want[k]), (where, k)


@functools.lru_cache(maxsize=None)
def _oracle(shape, shield):
    """The oracle's tape of a case, computed once: the per-step records and the episode counter at the end."""
    E, N = SHAPES[shape]
    oracle_env.set_math_mode(1)  # include/mm_math.h on both sides: bit-for-bit comparison
    try:
        env = oracle_env.OracleEnv(E, N, **_kw(shield))
        env.reset()
        return [_snap(env, env.step(a)) for a in _actions(E, N, STEPS, 7)]
    finally:
        oracle_env.set_math_mode(0)


@pytest.mark.parametrize("shield", list(SHIELDS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_env_respawns_in_the_oracle_tape(shape, shield):
    """(CPU) the case does what the parity test needs of it: every env ends an episode within the 120 steps."""
    tape = _oracle(shape, shield)
    assert bool((tape[-1]["env_i32"][abi.EP["EPISODE"]] >= 1).all())
    assert bool(torch.stack([r["done"] for r in tape]).any(0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shield", list(SHIELDS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rollout_against_oracle(shape, shield):
    E, N = SHAPES[shape]
    env = VecMergeEnv(E, N, device="cuda:0", **_kw(shield))
    env.reset()
    for t, (a, want) in enumerate(zip(_actions(E, N, STEPS, 7), _oracle(shape, shield))):
        _assert_same(_snap(env, env.step(a.cuda())), want, (shape, shield, t))
    env.poll_errors()
    env.close()


def _fresh_from(env, shield):
    """A fresh handle on a copy of env's present state."""
    other = VecMergeEnv(env.E, env.N, device="cuda:0", **_kw(shield))
    other.load_state_dict(env.state_dict())
    return other


def _check_against_fresh(env, shield, a, where):
    """env (whatever its carried planes hold) and a fresh handle on the same state take the same step."""
    fresh = _fresh_from(env, shield)
    got, want = _snap(env, env.step(a)), _snap(fresh, fresh.step(a))
    _assert_same(got, want, where)
    fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shield", list(SHIELDS))
@pytest.mark.parametrize("shape", ["E9_N8", "E5_N4"])
def test_stale_planes_step_like_a_fresh_handle(shape, shield):
    E, N = SHAPES[shape]
    acts = [a.cuda() for a in _actions(E, N, 12, 11)]
    env = VecMergeEnv(E, N, device="cuda:0", **_kw(shield))
    env.reset()
    _check_against_fresh(env, shield, acts[0], "first step of a fresh handle")
    for a in acts[1:3]:
        env.step(a)
    early = env.state_dict()
    # the caller writes x, heading and lane of two vehicles, taken from another env of the batch (valid poses)
    F, B = abi.F, abi.B
    for (e, v), (es, vs) in (((0, 1), (3, 0)), ((E - 1, N - 1), (2, 1))):
        for p in (F["X"], F["HEADING"]):
            env.f64[p, e, v] = env.f64[p, es, vs]
        env.u8[B["LANE"], e, v] = env.u8[B["LANE"], es, vs]
    _check_against_fresh(env, shield, acts[3], "after the caller's edit")
    for a in acts[4:6]:
        env.step(a)
    mask = torch.zeros(E, dtype=torch.uint8)
    mask[1::2] = 1
    env.reset(env_mask=mask)
    _check_against_fresh(env, shield, acts[6], "after a masked reset")
    for a in acts[7:9]:
        env.step(a)
    env.load_state_dict(early)  # a batch resumed from a saved state, in a handle whose planes describe a later one
    _check_against_fresh(env, shield, acts[9], "resumed from a saved state")
    # ... and the resumed batch goes on as the first run did from there
    again = VecMergeEnv(E, N, device="cuda:0", **_kw(shield))
    again.load_state_dict(early)
    again.step(acts[9])
    for a in acts[10:]:
        _assert_same(_snap(env, env.step(a)), _snap(again, again.step(a)), "after the resume")
    env.close()
    again.close()


@pytest.mark.gpu
def test_graph_of_four_steps_equals_eager():
    E, N = SHAPES["E9_N8"]
    acts = [a.cuda() for a in _actions(E, N, 9, 13)]
    eager = VecMergeEnv(E, N, device="cuda:0", **_kw("mass"))
    graph = VecMergeEnv(E, N, device="cuda:0", **_kw("mass"))
    eager.reset()
    graph.reset()
    slot = [torch.zeros_like(acts[0]) for _ in range(4)]  # the captured steps read their actions from here
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph.step(acts[0])  # warm-up, outside the capture
        eager.step(acts[0])
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(4):
            graph.step(slot[k])
    for rep in range(2):
        for k in range(4):
            slot[k].copy_(acts[1 + 4 * rep + k])
        g.replay()
        for k in range(4):
            res = eager.step(acts[1 + 4 * rep + k])
        torch.cuda.synchronize()
        _assert_same(_snap(graph, (graph.obs, graph.out["reward"], graph.out["done"], graph.out)), _snap(eager, res), ("replay", rep))
    eager.poll_errors()
    graph.poll_errors()
    eager.close()
    graph.close()
