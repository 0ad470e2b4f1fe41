"""MM_ROUNDS_PRIOR: the exact-mode MASS rounds of step_kernel start from the inactive QP's acceleration, and nothing changes.

The scripted batch of tests/test_rounds_prior_host.py (which replays the rounds from both seeds and counts the cases the batch
holds: an env without an active QP, a chain of active followers, the slow-LC bypass, constrain_adj with h3 binding, a
stopped leader, g0 <= 0) and the random steps around its scenes, on the device:

* every group size the loop is compiled for -- 16 x 8, 10 x 6 (6-lane rotation layout with idle tail lanes), 5 x 12 and
  5 x 9 in the 12-lane layout and, with debug_flags bit 1, in 16-lane groups, 16 x 4, 32 x 2 -- with three sub-steps per step
  (the product's configuration) and, at 16 x 8, with the one sub-step per step the host replay runs on;
* the kernel without the trace (the product's instantiation), the TRACE instantiation with its QP planes (rows, a, h0..h3,
  d, margin, status, headway per sub-step) and the literal sweep (debug_flags bit 0) of the same kernel: all bit-equal to
  the CPU oracle -- state planes, obs (f64), rewards, dones, the whole info dict;
* a handle resumed from the state planes saved right after the scenes were placed steps like the uninterrupted run;
* a captured graph of 4 steps over the scenes, replayed twice, equals the eager run;
* the sine lane from one sub-step to the next (the ramp tape of the host file: a vehicle on kb0, one crossing jk0 -> kb0 inside a
  step, one for which closest_lane takes its early-out, a vetoed lane change that commits candidate B): production and trace
  instantiation, parallel and literal sweep, bit-equal to the oracle.
"""
import pytest
import torch

import test_rounds_prior_host as H
from marl_mass_amd import VecMergeEnv

SHAPES, STEPS = H.SHAPES, H.STEPS
CASES = [(s, 3) for s in SHAPES] + [("E16_N8", 1)]


def _env(shape, nsub, **more):
    E, N = SHAPES[shape]
    flags = H.GPU_FLAGS.get(shape, 0) | more.pop("debug_flags", 0)
    return VecMergeEnv(E, N, device="cuda:0", **H.kw(nsub, debug_flags=flags, **more))


def _without_trace(rec):
    return {k: w for k, w in rec.items() if k != "trace"}


@pytest.mark.gpu
@pytest.mark.parametrize("shape,nsub", CASES)
def test_scripted_rollout_against_oracle_and_literal_sweep(shape, nsub):
    E, N = SHAPES[shape]
    plain, traced, lit = _env(shape, nsub), _env(shape, nsub, trace=True), _env(shape, nsub, trace=True, debug_flags=1)
    envs = (plain, traced, lit)
    for env in envs:
        env.reset()
    for t, st in enumerate(H.oracle_tape(shape, nsub)):
        a = st["act"].cuda()
        if t in H.SCRIPT_AT:
            for env in envs:
                H.script(env)
            assert H.same(traced.f64.cpu(), st["pre"]["f64"]) and H.same(traced.u8.cpu(), st["pre"]["u8"]), (shape, t, "the edit")
        H.assert_same(H.snap(plain, plain.step(a)), _without_trace(st["rec"]), (shape, nsub, t, "oracle"))
        H.assert_same(H.snap(traced, traced.step(a)), st["rec"], (shape, nsub, t, "oracle, with the trace"))
        H.assert_same(H.snap(lit, lit.step(a)), st["rec"], (shape, nsub, t, "literal sweep"))
    for env in envs:
        env.poll_errors()
        env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["E16_N8", "E10_N6"])
def test_resume_from_the_state_planes_with_the_scenes_placed(shape):
    tape = H.oracle_tape(shape, 3)
    at = H.SCRIPT_AT[0]
    env = _env(shape, 3)
    env.reset()
    for st in tape[:at]:
        env.step(st["act"].cuda())
    H.script(env)
    saved = env.state_dict()
    again = _env(shape, 3)
    again.load_state_dict(saved)
    for t, st in enumerate(tape[at:at + 5]):
        a = st["act"].cuda()
        got = H.snap(again, again.step(a))
        H.assert_same(got, H.snap(env, env.step(a)), (shape, "after the resume", t))
        H.assert_same(got, _without_trace(st["rec"]), (shape, "after the resume, oracle", t))
    env.poll_errors()
    again.poll_errors()
    env.close()
    again.close()


@pytest.mark.gpu
def test_graph_of_four_steps_over_the_scenes_equals_eager():
    shape, at = "E16_N8", H.SCRIPT_AT[0]
    acts = [st["act"].cuda() for st in H.oracle_tape(shape, 3)]
    eager, graph = _env(shape, 3), _env(shape, 3)
    eager.reset()
    graph.reset()
    slot = [torch.zeros_like(acts[0]) for _ in range(4)]  # the captured steps read their actions from here
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for a in acts[:at - 1]:  # warm-up, outside the capture
            graph.step(a)
            eager.step(a)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(4):
            graph.step(slot[k])
    first = at - 1
    for rep in range(2):
        H.script(graph)  # the scenes go in before either replay: both step them
        H.script(eager)
        for k in range(4):
            slot[k].copy_(acts[first + 4 * rep + k])
        g.replay()
        for k in range(4):
            res = eager.step(acts[first + 4 * rep + k])
        torch.cuda.synchronize()
        H.assert_same(H.snap(graph, (graph.obs, graph.out["reward"], graph.out["done"], graph.out)), H.snap(eager, res), ("replay", rep))
    eager.poll_errors()
    graph.poll_errors()
    eager.close()
    graph.close()


@pytest.mark.gpu
@pytest.mark.parametrize("debug_flags", [0, 1], ids=["parallel", "literal"])
@pytest.mark.parametrize("trace", [False, True], ids=["production", "trace"])
def test_the_sine_lane_from_sub_step_to_sub_step(trace, debug_flags):
    got = H.ramp_run(lambda E, N, **kw: VecMergeEnv(E, N, device="cuda:0", **kw), trace=trace, debug_flags=debug_flags)
    for t, (g, w) in enumerate(zip(got, H.ramp_oracle_tape())):
        H.assert_same(g, w if trace else _without_trace(w), (trace, debug_flags, t))

