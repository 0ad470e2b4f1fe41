"""The combined select forms and the early prologue loads of the fused step kernels (MM_CORNER_SELECTS, MM_ATAN_SELECTS,
MM_TRIG_SELECTS, MM_CLIP_SELECTS, MM_EARLY_LOADS) against the CPU oracle, bit for bit.

The batch is the placed one of tests/test_combined_forms_host.py, which counts from the oracle's planes that it holds vehicles
on the sine lane kb0, at the lane hand-overs and mid lane-change, a crashed vehicle (whose env is done and re-spawns in the same
launch, from the n_merge / episode the prologue read), speeds beyond + / - max, the lane-change clip at both ends and actions
outside 0 .. 4.  Every comparison is exact (equal bits, equal NaN positions, equal dtypes): every step's obs, rewards, dones,
info, every state plane and the env counters, and which steps latched an error.

* 8 envs x 8 CAVs MASS (one wave, every lane of it), 16 x 8 (two waves), 8 x 4, 8 x 2 and 8 x 8 HSS, all with the exact QP;
* float32 observations (the LDS-staged rows) for 8 x 8;
* a captured graph of the three steps after the caller's edit -- with the re-spawn inside the replay -- equals the eager run
  and the oracle.
"""
import pytest
import torch

import test_combined_forms_host as P
import test_scan_selects_host as H
from marl_mass_amd import VecMergeEnv

CASES = P.CASES


def _env(name, **more):
    E, N, _ = CASES[name]
    return VecMergeEnv(E, N, device="cuda:0", **P.kw(name, **more))


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
    got = P.run(env, E, N)
    want = P.oracle_tape(name)
    _compare(got, want, (name,))
    for t in P.SCRIPT_AT:  # the env with the crashed vehicle: done, and in its next episode when the launch returns
        ep = H.abi.EP["EPISODE"]
        assert int(got[t]["rec"]["env_i32"][ep, 3]) == int(got[t]["pre"]["env_i32"][ep, 3]) + 1
        assert bool(got[t]["rec"]["done"][3])
    env.close()


@pytest.mark.gpu
def test_float32_observations():
    name = "E8_N8_mass"
    E, N, _ = CASES[name]
    import oracle_env
    oracle_env.set_math_mode(1)
    try:
        want = P.run(oracle_env.OracleEnv(E, N, **P.kw(name, obs_f64=False)), E, N)
    finally:
        oracle_env.set_math_mode(0)
    env = _env(name, obs_f64=False)
    _compare(P.run(env, E, N), want, (name, "float32 rows"))
    env.close()


@pytest.mark.gpu
def test_graph_with_the_respawn_inside_equals_eager():
    name = "E16_N8_mass"
    E, N, _ = CASES[name]
    acts = [a.clamp(0, 4).cuda() for a in P.actions(E, N)]  # (no latch inside the replay: the bad actions have their own test)
    at = P.SCRIPT_AT[0]
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
    P.script(eager)
    P.script(graph)
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
    # the oracle, with the same clamped actions
    import oracle_env
    oracle_env.set_math_mode(1)
    try:
        cpu = oracle_env.OracleEnv(E, N, **P.kw(name))
        cpu.reset()
        for t in range(at + 3):
            if t == at:
                P.script(cpu)
            res_c = cpu.step(acts[t].cpu())
        H.assert_same(got, H.snap(cpu, res_c), (name, "oracle"))
    finally:
        oracle_env.set_math_mode(0)
    eager.poll_errors()
    graph.poll_errors()
    eager.close()
    graph.close()
