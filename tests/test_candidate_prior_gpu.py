"""The candidate the veto prior picks is the main pass's, the other one is evaluated lazily (kPrimary in step_kernel): the
fused exact-mode CAV-only kernels of the 2- / 4- / 8-lane groups, without the trace.

Nothing about the results may change -- the same candidates with the same bits, only computed at another time:

* parity -- 120 auto-resetting steps on the lane-change-heavy tapes of tests/test_candidate_prior_host.py (which counts the
  cases they contain: prior "vetoed" and the veto holds / is lifted, prior "safe" and the veto fires, crashed vehicles)
  against the CPU oracle AND against the same kernel in its literal sweep (debug_flags = 1, where the prior picks nothing
  and every missing candidate is evaluated for the sweep), bit for bit: state planes, obs (f64), rewards, dones, the whole
  info dict.  MASS and HSS at 9 x 8 (two waves, the second partly empty), 5 x 4, 3 x 2, and 5 x 5 (the 6-lane rotation
  layout, which keeps the old code);
* the crash tape -- vehicles the caller marked crashed step with their shields on (crashed => needB under either prior);
* the "unsafe" tapes -- 5 x 4 and 3 x 2 with IS_LC_SAFE cleared by the caller before each of forty steps, so that the 4- and
  2-lane kernels evaluate A lazily too (their random tapes hold no lifted veto);
* state -- a handle resumed from a checkpoint taken mid-episode while vetoed lanes exist steps like the uninterrupted run;
* a captured graph of 4 steps, replayed twice, equals the eager run.
"""
import pytest
import torch

import test_candidate_prior_host as H
from marl_mass_amd import VecMergeEnv, _cabi as abi

SHAPES, SHIELDS, STEPS = H.SHAPES, H.SHIELDS, H.STEPS


def _env(shape, shield, **more):
    E, N = SHAPES[shape]
    return VecMergeEnv(E, N, device="cuda:0", **H.kw(shield, **more))


@pytest.mark.gpu
@pytest.mark.parametrize("shield", list(SHIELDS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rollout_against_oracle_and_literal_sweep(shape, shield):
    E, N = SHAPES[shape]
    env, lit = _env(shape, shield), _env(shape, shield, debug_flags=1)
    env.reset()
    lit.reset()
    for t, (a, st) in enumerate(zip(H.actions(E, N, STEPS), H.oracle_tape(shape, shield))):
        a = a.cuda()
        got = H.snap(env, env.step(a))
        H.assert_same(got, st["rec"], (shape, shield, t, "oracle"))
        H.assert_same(H.snap(lit, lit.step(a)), got, (shape, shield, t, "literal sweep"))
    env.poll_errors()
    lit.poll_errors()
    env.close()
    lit.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shield", list(SHIELDS))
def test_crashed_vehicles_with_their_shields_on(shield):
    E, N = SHAPES["E9_N8"]
    acts = [a.cuda() for a in H.actions(E, N, H.CRASH_AFTER + 1)]
    env, lit = _env("E9_N8", shield), _env("E9_N8", shield, debug_flags=1)
    for e in (env, lit):
        e.reset()
        for a in acts[:-1]:
            e.step(a)
        H.mark_crashed(e)
    want = H.oracle_crash_tape(shield)[0]
    assert torch.equal(env.u8.cpu(), want["pre"]["u8"])  # the edit lands on the state the oracle edited
    got = H.snap(env, env.step(acts[-1]))
    H.assert_same(got, want["rec"], (shield, "oracle"))
    H.assert_same(H.snap(lit, lit.step(acts[-1])), got, (shield, "literal sweep"))
    env.poll_errors()
    env.close()
    lit.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shield", list(SHIELDS))
@pytest.mark.parametrize("shape", list(H.UNSAFE_SHAPES))
def test_vetoes_lifted_after_the_callers_edit(shape, shield):
    E, N = SHAPES[shape]
    env, lit = _env(shape, shield), _env(shape, shield, debug_flags=1)
    env.reset()
    lit.reset()
    want = iter(H.oracle_unsafe_tape(shape, shield))
    for t, a in enumerate(H.actions(E, N, H.UNSAFE_TO)):
        a = a.cuda()
        if t < H.UNSAFE_FROM:
            env.step(a)
            lit.step(a)
            continue
        H.mark_unsafe(env)
        H.mark_unsafe(lit)
        got = H.snap(env, env.step(a))
        H.assert_same(got, next(want)["rec"], (shape, shield, t, "oracle"))
        H.assert_same(H.snap(lit, lit.step(a)), got, (shape, shield, t, "literal sweep"))
    env.poll_errors()
    env.close()
    lit.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shield", list(SHIELDS))
@pytest.mark.parametrize("shape", ["E9_N8", "E5_N4"])
def test_resume_from_a_checkpoint_with_vetoed_lanes(shape, shield):
    E, N = SHAPES[shape]
    acts = [a.cuda() for a in H.actions(E, N, 90)]
    env = _env(shape, shield)
    env.reset()
    B, SAFE = abi.B, abi.FLAG_IS_LC_SAFE
    saved, at = None, None
    for t, a in enumerate(acts[:80]):
        env.step(a)
        # mid-episode, in the merging zone, and some shielded vehicle's last decision was a veto: the prior picks B for it in
        # the next step if its lane change goes on
        live = (env.u8[B["KIND"]] != 0) & (env.u8[B["HIST_LEN"]] >= 2)
        vetoed = live & ((env.u8[B["FLAGS"]] & SAFE) == 0)
        if t >= 45 and bool(vetoed.any()):
            saved, at = env.state_dict(), t
            break
    assert saved is not None, "the tape holds no vetoed lane in steps 45..79"
    again = _env(shape, shield)
    again.load_state_dict(saved)
    for t, a in enumerate(acts[at + 1: at + 9]):
        H.assert_same(H.snap(again, again.step(a)), H.snap(env, env.step(a)), (shape, shield, "after the resume", t))
    env.poll_errors()
    again.poll_errors()
    env.close()
    again.close()


@pytest.mark.gpu
def test_graph_of_four_steps_equals_eager():
    E, N = SHAPES["E9_N8"]
    acts = [a.cuda() for a in H.actions(E, N, 9 + 45)][45:]  # (in the merging zone: the shields are on, lane changes under way)
    lead = [a.cuda() for a in H.actions(E, N, 45)]
    eager, graph = _env("E9_N8", "mass"), _env("E9_N8", "mass")
    eager.reset()
    graph.reset()
    slot = [torch.zeros_like(acts[0]) for _ in range(4)]  # the captured steps read their actions from here
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for a in lead + acts[:1]:  # warm-up, outside the capture
            graph.step(a)
            eager.step(a)
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
        H.assert_same(H.snap(graph, (graph.obs, graph.out["reward"], graph.out["done"], graph.out)), H.snap(eager, res), ("replay", rep))
    eager.poll_errors()
    graph.poll_errors()
    eager.close()
    graph.close()
