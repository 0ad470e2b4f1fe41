"""The select forms of the sweep rank and of observe()'s neighbour order (MM_SCAN_SELECTS) against the CPU oracle, bit for bit.

The batch is the scripted one of tests/test_scan_selects_host.py, which counts from the oracle's state planes that it holds
rank ties in both index orders, absent partners, neighbours at equal keys, more than four neighbours in sight, keys that are
+inf (and two that tie) and a vehicle that is not controlled.  Every comparison is exact (H.assert_same: equal bits, equal
NaN positions, equal dtypes), as in the other oracle parity tests; nothing here has a tolerance.

* the scripted batch -- per step obs, rewards, dones, the info dict and every state plane, and after each of the caller's edits
  the stand-alone observe() of the placed state -- for MASS and HSS with the exact QP, every group size (2, 3 of 4, 4, 6, 8,
  and 12 / 9 of 16 through debug_flags bit 1), the mixed-traffic batch (general kernels), and the literal sweep
  (debug_flags bit 0) against the parallel form;
* the interior-point QP, fused and as the split step (debug_flags bit 3), whose phase kernels carry the same rank and observe();
* float32 observations (the LDS-staged row writes) for an 8-, a 4-of-3- and a 6-lane group;
* a random rollout of a ragged mixed-traffic batch (drawn counts: absent and uncontrolled slots that differ from env to env);
* a captured graph of four steps equals the eager run.
"""
import pytest
import torch

import oracle_env
import test_scan_selects_host as H
from marl_mass_amd import VecMergeEnv

SHAPES, SHIELDS = H.SHAPES, H.SHIELDS


def _env(shape, shield, flags=0, **more):
    E, N, _ = SHAPES[shape]
    return VecMergeEnv(E, N, device="cuda:0", **H.kw(shape, shield, debug_flags=H.GPU_FLAGS.get(shape, 0) | flags, **more))


def _compare(got, want, where):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        H.assert_same(g["rec"], w["rec"], where + (t, "step"))
        assert (g["placed"] is None) == (w["placed"] is None)
        if w["placed"] is not None:
            H.assert_same(g["placed"], w["placed"], where + (t, "observe() of the placed state"))


@pytest.mark.gpu
@pytest.mark.parametrize("shield", list(SHIELDS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_scripted_batch_against_oracle_and_literal_sweep(shape, shield):
    E, N, _ = SHAPES[shape]
    env, lit = _env(shape, shield), _env(shape, shield, flags=1)
    got = H.run(env, E, N)
    _compare(got, H.oracle_tape(shape, shield), (shape, shield, "oracle"))
    _compare(H.run(lit, E, N), got, (shape, shield, "literal sweep"))
    env.poll_errors()
    lit.poll_errors()
    env.close()
    lit.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [4, 8], ids=["fused", "split"])  # (debug_flags bit 2 keeps the fused kernel, bit 3 forces the split step)
@pytest.mark.parametrize("shield", list(SHIELDS))
@pytest.mark.parametrize("shape", ["E5_N8", "E5_N3", "E5_N6", "E5_N4_H1"])
def test_interior_point_step(shape, shield, flags):
    E, N, _ = SHAPES[shape]
    env = _env(shape, shield, flags=flags, qp_solver="ipm")
    _compare(H.run(env, E, N), H.oracle_tape(shape, shield, "ipm"), (shape, shield, "ipm", flags))
    env.poll_errors()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["E5_N8", "E5_N3", "E5_N6", "E5_N4_H1"])
def test_float32_observations(shape):
    E, N, _ = SHAPES[shape]
    env = _env(shape, "mass", obs_f64=False)
    _compare(H.run(env, E, N), H.oracle_tape(shape, "mass", "exact", False), (shape, "float32 rows"))
    env.poll_errors()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shield", list(SHIELDS))
def test_random_rollout_of_a_ragged_mixed_batch(shield):
    """Drawn vehicle counts (traffic_density 2, mixed traffic): 5 envs of up to 8 slots whose numbers of controlled, uncontrolled
    and absent vehicles differ from env to env; 12 steps from the reset, no edit."""
    E, N = 5, 8
    kw = dict(env_id="merge-multi-agent-v1",
              config={"safety_guarantee": SHIELDS[shield], "HEADWAY_TIME": 0.5, "traffic_density": 2, "traffic_type": "mixed",
                      "mixed_traffic": True},
              cbf_eta=0.03125, cbf_tau=0.5, qp_solver="exact", obs_f64=True, auto_reset=True, seed=161, draw_counts=True)
    oracle_env.set_math_mode(1)
    try:
        gpu, cpu = VecMergeEnv(E, N, device="cuda:0", **kw), oracle_env.OracleEnv(E, N, **kw)
        og, _ = gpu.reset()
        oc, _ = cpu.reset()
        assert H.same(og.cpu(), oc) and H.same(gpu.u8.cpu(), cpu.u8)
        kinds = set()
        for t, a in enumerate(H.actions(E, N, steps=12, seed=59)):
            kinds |= set(cpu.u8[H.abi.B["KIND"]].flatten().tolist())
            H.assert_same(H.snap(gpu, gpu.step(a.cuda())), H.snap(cpu, cpu.step(a)), (shield, t))
        assert kinds == {0, 1, 2}, kinds  # absent, controlled and uncontrolled vehicles all occurred
    finally:
        oracle_env.set_math_mode(0)
    gpu.poll_errors()
    gpu.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["E5_N8", "E5_N9_G16"])
def test_graph_of_four_steps_equals_eager(shape):
    E, N, _ = SHAPES[shape]
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
    H.script(eager)  # the four steps after the caller's edit: the ties play out inside the replay
    H.script(graph)
    for k in range(4):
        slot[k].copy_(acts[at + k])
    g.replay()
    for k in range(4):
        res = eager.step(acts[at + k])
    torch.cuda.synchronize()
    got = H.snap(graph, (graph.obs, graph.out["reward"], graph.out["done"], graph.out))
    H.assert_same(got, H.snap(eager, res), (shape, "replay"))
    H.assert_same(got, H.oracle_tape(shape, "mass")[at + 3]["rec"], (shape, "oracle"))
    eager.poll_errors()
    graph.poll_errors()
    eager.close()
    graph.close()
