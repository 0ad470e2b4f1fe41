"""The relation word of the pose codes (MM_RELATION_WORD: the owner of a pose publishes the lane-pair relation that
relate_word() reads, in the 8-lane kernels) against the CPU oracle bit for bit, and the same batch through the 4- and 2-lane
kernels, which derive the relation from the lanes as before.

The batch is the placed one of tests/test_relation_word_host.py -- 16 envs (two waves at 8 vehicles) that hold every (reader
pair, owner pair) combination with and without a corner bit in the owner's code -- stepped MASS and HSS through N = 8, 4, 2.
Every comparison is exact (equal bits, equal NaN positions, equal dtypes): each step's obs, rewards, dones, info, every state
plane (the flags plane with IS_LC_SAFE among them) and the env counters.

* the placed batch against the oracle, six cases;
* debug_flags bit 0 (the literal sweep, which derives the relation from the lanes) on the same batch: the same bits;
* the carried pose: the step after the edit's step takes its pose codes from the previous launch (PoseBuf) and forms the word
  again from the carried lanes -- it equals the step of a fresh handle on the same state, which carries nothing;
* a captured graph of the steps from the edit on equals the eager run and the oracle.
"""
import pytest
import torch

import test_relation_word_host as R
import test_scan_selects_host as H
from marl_mass_amd import VecMergeEnv

CASES = R.CASES


def _env(name, **more):
    E, N, _ = CASES[name]
    return VecMergeEnv(E, N, device="cuda:0", **R.kw(name, **more))


def _compare(got, want, where):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        H.assert_same(g["rec"], w["rec"], where + (t,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_placed_batch_against_oracle(name):
    E, N, _ = CASES[name]
    env = _env(name)
    got = R.run(env, E, N)
    assert "u8" in got[0]["rec"] and "f64" in got[0]["rec"]
    _compare(got, R.oracle_tape(name), (name,))
    env.poll_errors()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["E16_N8_mass", "E16_N4_hss"])
def test_literal_sweep_gives_the_same_bits(name):
    E, N, _ = CASES[name]
    env = _env(name, debug_flags=1)
    _compare(R.run(env, E, N), R.oracle_tape(name), (name, "literal sweep"))
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["E16_N8_mass", "E16_N2_hss"])
def test_carried_pose_forms_the_word_again(name):
    E, N, _ = CASES[name]
    acts = [a.cuda() for a in R.actions(E, N)]
    env = _env(name)
    env.reset()
    for t in range(R.SCRIPT_AT):
        env.step(acts[t])
    R.script(env)
    env.step(acts[R.SCRIPT_AT])  # (the edit invalidates what the handle carried: this launch derives every pose code)
    tape = R.oracle_tape(name)
    for t in range(R.SCRIPT_AT + 1, R.STEPS):  # these launches take the carried pose
        fresh = _env(name)
        fresh.load_state_dict(env.state_dict())  # the same state in a handle that carries nothing
        got = H.snap(env, env.step(acts[t]))
        H.assert_same(got, H.snap(fresh, fresh.step(acts[t])), (name, "fresh handle", t))
        H.assert_same(got, tape[t]["rec"], (name, "oracle", t))
        fresh.close()
    env.close()


@pytest.mark.gpu
def test_graph_from_the_edit_on_equals_eager():
    name = "E16_N8_mass"
    E, N, _ = CASES[name]
    acts = [a.cuda() for a in R.actions(E, N)]
    at, n = R.SCRIPT_AT, R.STEPS - R.SCRIPT_AT
    eager, graph = _env(name), _env(name)
    eager.reset()
    graph.reset()
    slot = [torch.zeros_like(acts[0]) for _ in range(n)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for a in acts[:at]:  # warm-up, outside the capture
            graph.step(a)
            eager.step(a)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(n):
            graph.step(slot[k])
    R.script(eager)
    R.script(graph)
    for k in range(n):
        slot[k].copy_(acts[at + k])
    g.replay()
    for k in range(n):
        res = eager.step(acts[at + k])
    torch.cuda.synchronize()
    got = H.snap(graph, (graph.obs, graph.out["reward"], graph.out["done"], graph.out))
    H.assert_same(got, H.snap(eager, res), (name, "replay"))
    H.assert_same(got, R.oracle_tape(name)[-1]["rec"], (name, "oracle"))
    eager.poll_errors()
    graph.poll_errors()
    eager.close()
    graph.close()
