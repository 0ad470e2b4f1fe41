"""The partner bits of the fused step kernels (MM_PARTNER_BITS: what a lane sees of a partner from the rank scan and a fixed post
image instead of rank words) against the CPU oracle, bit for bit.

The batch is the placed one of tests/test_partner_bits_host.py, which counts from the oracle's planes and trace that it holds a
pair of live vehicles at bit-equal x in both index orders, an env that ends in sub-step 0 or 1 of a step, a crashed vehicle,
a veto that fires on a lane that started from A, a lifted veto of a lane that started from B with a follower behind it (a second
pass reads the re-published post image) and a re-spawn.  Every comparison is exact (equal bits, equal NaN positions, equal
dtypes): every step's obs, rewards, dones, info, every state plane and the env counters, and which steps latched an error.

* float32 rows for 8 envs x 8 CAVs MASS (one wave, every lane), 16 x 8, 9 x 8 (ragged second wave), 8 x 7 (N < G: an absent
  partner), 8 x 4, 8 x 2, 8 x 8 HSS; float64 rows for 8 x 8;
* debug_flags bit 0 (the literal sweep) on the same batch: the same bits;
* a batch resumed in a fresh handle steps like the uninterrupted one and like the oracle;
* a captured graph of the three steps after the caller's edit -- with the re-spawn inside the replay -- equals the eager run
  and the oracle.
"""
import pytest
import torch

import oracle_env
import test_partner_bits_host as B
import test_scan_selects_host as H
from marl_mass_amd import VecMergeEnv

CASES = B.CASES


def _env(name, **more):
    E, N, _ = CASES[name]
    return VecMergeEnv(E, N, device="cuda:0", **B.kw(name, **more))


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
    got = B.run(env, E, N)
    assert got[0]["rec"]["obs"].dtype == torch.float32
    want = B.oracle_tape(name)
    _compare(got, want, (name,))
    assert [g["latched"] for g in got] == [t in B.SCRIPT_AT for t in range(B.STEPS)]  # the steps that latch: the bad actions'
    ep = H.abi.EP["EPISODE"]
    for t in B.SCRIPT_AT:  # the env with the crashed vehicle: done, and in its next episode when the launch returns
        assert int(got[t]["rec"]["env_i32"][ep, 3]) == int(got[t]["pre"]["env_i32"][ep, 3]) + 1
        assert bool(got[t]["rec"]["done"][3])
    env.close()


@pytest.mark.gpu
def test_float64_rows():
    name = "E8_N8_mass"
    E, N, _ = CASES[name]
    env = _env(name, obs_f64=True)
    got = B.run(env, E, N)
    assert got[0]["rec"]["obs"].dtype == torch.float64
    _compare(got, B.oracle_tape(name, True), (name, "float64 rows"))
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["E9_N8_mass", "E8_N4_mass", "E8_N2_mass", "E8_N8_hss"])
def test_literal_sweep_gives_the_same_bits(name):
    E, N, _ = CASES[name]
    env = _env(name, debug_flags=1)
    _compare(B.run(env, E, N), B.oracle_tape(name), (name, "literal sweep"))
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["E9_N8_mass", "E8_N4_mass"])
def test_resumed_batch(name):
    E, N, _ = CASES[name]
    acts = [a.cuda() for a in B.actions(E, N)]
    at = B.SCRIPT_AT[1]
    env = _env(name)
    env.reset()
    for t, a in enumerate(acts[:at]):
        if t in B.SCRIPT_AT:
            B.script(env, t)
        env.step(a)
    B.script(env, at)
    again = _env(name)
    again.load_state_dict(env.state_dict())  # the scenes as the caller left them; this handle carries nothing yet
    tape = B.oracle_tape(name)
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
    acts = [a.clamp(0, 4).cuda() for a in B.actions(E, N)]  # (no latch inside the replay: the bad actions have their own test)
    at = B.SCRIPT_AT[1]  # (the edit that clears IS_LC_SAFE: the replay holds the lifted vetoes)
    eager, graph = _env(name), _env(name)
    eager.reset()
    graph.reset()
    slot = [torch.zeros_like(acts[0]) for _ in range(3)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for t, a in enumerate(acts[:at]):  # warm-up, outside the capture
            if t in B.SCRIPT_AT:
                B.script(graph, t)
                B.script(eager, t)
            graph.step(a)
            eager.step(a)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(3):
            graph.step(slot[k])
    B.script(eager, at)
    B.script(graph, at)
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
        cpu = oracle_env.OracleEnv(E, N, **B.kw(name))
        cpu.reset()
        for t in range(at + 3):
            if t in B.SCRIPT_AT:
                B.script(cpu, t)
            res_c = cpu.step(acts[t].cpu())
        H.assert_same(got, H.snap(cpu, res_c), (name, "oracle"))
    finally:
        oracle_env.set_math_mode(0)
    eager.poll_errors()
    graph.poll_errors()
    eager.close()
    graph.close()
