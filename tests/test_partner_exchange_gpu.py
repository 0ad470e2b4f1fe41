"""The partner exchanges of the step kernels (dppx_i: the DPP row permutations every power-of-two group kernel shares, now with
bound_ctrl and no `old` operand; the sweep rank; the collision pre-check) against the CPU oracle, bit for bit.

The batch is the scripted one of tests/test_partner_exchange_host.py, which counts from the oracle's trace that it holds a
near pair that does not touch, a colliding pair, a vehicle at the obstacle, a rank tie, an episode that ends in the first
sub-step and waves without any near pair.  12 steps per case, MASS and HSS with the exact QP:

* parity -- obs (f64), rewards, dones, the info dict and every state plane against the oracle, and the literal sweep
  (debug_flags bit 0) against the parallel form, for 2-, 4-, 8- and 16-lane groups with and without absent lanes (the
  16-lane groups -- row_ror:8, row_mirror -- through debug_flags bit 1: an env holds at most 12 vehicles, and 9..12 step in
  the rotation layout otherwise) and the 6-lane rotation layout, which does not use the helper and must be untouched;
* a batch resumed from a checkpoint taken right after the caller's second edit steps like the uninterrupted one;
* a captured graph of four steps equals the eager run.
"""
import pytest
import torch

import test_partner_exchange_host as H
from marl_mass_amd import VecMergeEnv

SHAPES, SHIELDS = H.SHAPES, H.SHIELDS


def _env(shape, shield, flags=0):
    E, N = SHAPES[shape]
    return VecMergeEnv(E, N, device="cuda:0", **H.kw(shield, debug_flags=H.GPU_FLAGS.get(shape, 0) | flags))


@pytest.mark.gpu
@pytest.mark.parametrize("shield", list(SHIELDS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_scripted_batch_against_oracle_and_literal_sweep(shape, shield):
    E, N = SHAPES[shape]
    env, lit = _env(shape, shield), _env(shape, shield, flags=1)
    env.reset()
    lit.reset()
    for t, (a, st) in enumerate(zip(H.actions(E, N), H.oracle_tape(shape, shield))):
        a = a.cuda()
        if t in H.SCRIPT_AT:
            H.script(env)
            H.script(lit)
        got = H.snap(env, env.step(a))
        H.assert_same(got, st["rec"], (shape, shield, t, "oracle"))
        H.assert_same(H.snap(lit, lit.step(a)), got, (shape, shield, t, "literal sweep"))
    env.poll_errors()
    lit.poll_errors()
    env.close()
    lit.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shield", list(SHIELDS))
@pytest.mark.parametrize("shape", ["E9_N7", "E5_N4", "E5_N12_G16"])
def test_resumed_batch(shape, shield):
    E, N = SHAPES[shape]
    acts = [a.cuda() for a in H.actions(E, N)]
    at = H.SCRIPT_AT[1]
    env = _env(shape, shield)
    env.reset()
    for t, a in enumerate(acts[:at]):
        if t in H.SCRIPT_AT:
            H.script(env)
        env.step(a)
    H.script(env)
    again = _env(shape, shield)
    again.load_state_dict(env.state_dict())  # the scenes as the caller left them: near pairs, the overlap, the tie
    tape = H.oracle_tape(shape, shield)
    for t, a in enumerate(acts[at:], start=at):
        got = H.snap(again, again.step(a))
        H.assert_same(got, H.snap(env, env.step(a)), (shape, shield, "after the resume", t))
        H.assert_same(got, tape[t]["rec"], (shape, shield, "oracle", t))
    env.poll_errors()
    again.poll_errors()
    env.close()
    again.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["E9_N8", "E5_N9_G16"])
def test_graph_of_four_steps_equals_eager(shape):
    E, N = SHAPES[shape]
    acts = [a.cuda() for a in H.actions(E, N)]
    at = H.SCRIPT_AT[0]
    eager, graph = _env(shape, "mass"), _env(shape, "mass")
    eager.reset()
    graph.reset()
    slot = [torch.zeros_like(acts[0]) for _ in range(4)]  # the captured steps read their actions from here
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for a in acts[:at]:  # warm-up, outside the capture
            graph.step(a)
            eager.step(a)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(4):
            graph.step(slot[k])
    H.script(eager)  # the four steps after the caller's edit: the scenes play out inside the replay
    H.script(graph)
    for k in range(4):
        slot[k].copy_(acts[at + k])
    g.replay()
    for k in range(4):
        res = eager.step(acts[at + k])
    torch.cuda.synchronize()
    got = H.snap(graph, (graph.obs, graph.out["reward"], graph.out["done"], graph.out))
    H.assert_same(got, H.snap(eager, res), (shape, "replay"))
    H.assert_same({k: got[k] for k in ("f64", "u8", "env_i32")},
                  {k: H.oracle_tape(shape, "mass")[at + 3]["rec"][k] for k in ("f64", "u8", "env_i32")}, (shape, "oracle"))
    eager.poll_errors()
    graph.poll_errors()
    eager.close()
    graph.close()
