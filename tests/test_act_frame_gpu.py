"""The act selects, the pose-code heading bits and the wide observation copy-out of the fused step kernels (MM_ACT_FRAME,
MM_POSE_HBITS, MM_OBS_WIDE) against the CPU oracle, bit for bit.

The batch is the placed one of tests/test_act_frame_host.py, which counts from the oracle's planes that it holds vehicles on
the sine lane kb0 and at its hand-over, vehicles off kb0 next to them, partners on either side in y and level, headings on
both sides of and exactly on both thresholds of relate(), such headings at steps that carry the pose code, and a re-spawn in
the step after the edit.  Every comparison is exact (equal bits, equal NaN positions, equal dtypes): every step's obs,
rewards, dones, info, every state plane and the env counters, and which steps latched an error.

* float32 rows (the copy-out under test) for 8 envs x 8 CAVs MASS (one wave, every lane busy: the 16-byte copy-out), 16 x 8,
  9 x 8 (the second wave holds one env: the ragged loop), 8 x 7 in 8-lane groups (N < G: the loop), 8 x 4, 8 x 2, 8 x 8 HSS;
* float64 rows for 8 x 8;
* a batch resumed in a fresh handle (whose first step derives the pose code, the later ones carry it) steps like the
  uninterrupted one and like the oracle;
* a captured graph of the three steps after the caller's edit -- with the re-spawn inside the replay -- equals the eager run
  and the oracle.
"""
import pytest
import torch

import oracle_env
import test_act_frame_host as A
import test_combined_forms_host as P
import test_scan_selects_host as H
from marl_mass_amd import VecMergeEnv

CASES = A.CASES


def _env(name, **more):
    E, N, _ = CASES[name]
    return VecMergeEnv(E, N, device="cuda:0", **A.kw(name, **more))


def _compare(got, want, where):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        H.assert_same(g["rec"], w["rec"], where + (t,))
        assert g["latched"] == w["latched"], where + (t, "latch")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_placed_batch_against_oracle(name):
    E, N, _ = CASES[name]
    env = _env(name)
    got = A.run(env, E, N)
    assert got[0]["rec"]["obs"].dtype == torch.float32
    _compare(got, A.oracle_tape(name), (name,))
    ep = H.abi.EP["EPISODE"]
    for t in A.SCRIPT_AT:  # the env with the crashed vehicle: done, and in its next episode when the launch returns
        assert int(got[t]["rec"]["env_i32"][ep, 3]) == int(got[t]["pre"]["env_i32"][ep, 3]) + 1
        assert bool(got[t]["rec"]["done"][3])
    env.close()


@pytest.mark.gpu
def test_float64_rows():
    name = "E8_N8_mass"
    E, N, _ = CASES[name]
    env = _env(name, obs_f64=True)
    got = A.run(env, E, N)
    assert got[0]["rec"]["obs"].dtype == torch.float64
    _compare(got, A.oracle_tape(name, True), (name, "float64 rows"))
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["E9_N8_mass", "E8_N4_mass"])
def test_resumed_batch(name):
    E, N, _ = CASES[name]
    acts = [a.cuda() for a in P.actions(E, N)]
    at = A.SCRIPT_AT[1]
    env = _env(name)
    env.reset()
    for t, a in enumerate(acts[:at]):
        if t in A.SCRIPT_AT:
            A.script(env)
        env.step(a)
    A.script(env)
    again = _env(name)
    again.load_state_dict(env.state_dict())  # the scenes as the caller left them; this handle carries nothing yet
    tape = A.oracle_tape(name)
    for t, a in enumerate(acts[at:], start=at):
        got = H.snap(again, again.step(a))
        H.assert_same(got, H.snap(env, env.step(a)), (name, "after the resume", t))
        H.assert_same(got, tape[t]["rec"], (name, "oracle", t))
    env.close()
    again.close()


@pytest.mark.gpu
def test_graph_with_the_respawn_inside_equals_eager():
    name = "E16_N8_mass"
    E, N, _ = CASES[name]
    acts = [a.clamp(0, 4).cuda() for a in P.actions(E, N)]  # (no latch inside the replay: the bad actions have their own test)
    at = A.SCRIPT_AT[0]
    eager, graph = _env(name), _env(name)
    eager.reset()
    graph.reset()
    slot = [torch.zeros_like(acts[0]) for _ in range(3)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for a in acts[:at]:  # warm-up, outside the capture
            graph.step(a)
            eager.step(a)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(3):
            graph.step(slot[k])
    A.script(eager)
    A.script(graph)
    ep = H.abi.EP["EPISODE"]
    before = int(graph.env_i32[ep, 3])
    for k in range(3):
        slot[k].copy_(acts[at + k])
    g.replay()
    for k in range(3):
        res = eager.step(acts[at + k])
    torch.cuda.synchronize()
    got = H.snap(graph, (graph.obs, graph.out["reward"], graph.out["done"], graph.out))
    H.assert_same(got, H.snap(eager, res), (name, "replay"))
    assert int(graph.env_i32[ep, 3]) == before + 1  # the crashed env re-spawned inside the replay
    oracle_env.set_math_mode(1)  # the oracle, with the same clamped actions
    try:
        cpu = oracle_env.OracleEnv(E, N, **A.kw(name))
        cpu.reset()
        for t in range(at + 3):
            if t == at:
                A.script(cpu)
            res_c = cpu.step(acts[t].cpu())
        H.assert_same(got, H.snap(cpu, res_c), (name, "oracle"))
    finally:
        oracle_env.set_math_mode(0)
    eager.poll_errors()
    graph.poll_errors()
    eager.close()
    graph.close()
