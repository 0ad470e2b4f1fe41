"""The hidden-512 actor without a GPU: the binding surface of mm_policy_wide_act, the resource budget of its translation unit,
DeviceRollout on the CPU oracle (which has no twin of the entry), and the conditions on the INPUTS of every case that
test_policy_wide_gpu.py runs on the device -- computed with the numpy Philox and the float64 network, never with code under
test."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

import oracle_env
import policy_wide_util as W
from marl_mass_amd import _cabi
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork, DeviceRollout

REPO = W.REPO
CSRC = os.path.join(REPO, "marl-mass_amd", "csrc")


def test_binding_surface():
    """libmm_hip.so exports mm_policy_wide_act as an optional symbol outside include/mm_abi.h's list, CLib binds it with
    mm_policy_act's argument types, and the oracle has no twin."""
    from marl_mass_amd import hip_library
    hip = hip_library()
    assert hip.has_policy_wide and hasattr(ctypes.CDLL(os.path.join(CSRC, "libmm_hip.so")), "mm_policy_wide_act")
    assert hip.lib.mm_policy_wide_act.argtypes == hip.lib.mm_policy_act.argtypes and hip.lib.mm_policy_wide_act.restype is ctypes.c_int32
    hip.require_policy_wide()
    assert "mm_policy_wide_act" not in _cabi.CLib.SYMBOLS
    orc = oracle_env.library()
    assert not orc.has_policy_wide
    try:
        orc.require_policy_wide()
    except NotImplementedError as e:
        assert "mm_policy_wide_act" in str(e)
    else:
        raise AssertionError("the oracle cannot serve the fused hidden-512 actor")


def test_header_declares_the_bound_symbol():
    txt = open(W.HEADER).read()
    decl = re.search(r"int32_t mm_policy_wide_act\(([^;]*)\);", txt)
    assert decl, "include/mm_policy_wide.h declares mm_policy_wide_act"
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert len(args) == 16 == len(_cabi.CLib(os.path.join(CSRC, "libmm_hip.so")).lib.mm_policy_wide_act.argtypes)
    assert args[0] == "const float *obs" and args[9] == "int32_t hidden" and args[-1] == "MMStream stream"
    assert W.TILE == 32 and W.WAVES >= 1 and W.MAX_GRID >= 1 and W.W2_ALIGN == 16
    abi_txt = open(os.path.join(REPO, "include", "mm_abi.h")).read()
    assert "mm_policy_wide_act" in abi_txt and "reference's only" not in abi_txt  # (128 is not the reference's only hidden size)


def test_kernel_resources(tmp_path):
    """Every kernel of mm_policy_wide.o: zero VGPR spills, zero scratch, LDS within a CU's 160 KiB, and what
    profiles/policy_wide/kernel_resources.json records is what the build gives."""
    subprocess.check_call(["make", "-C", CSRC, "mm_policy_wide.o"], stdout=subprocess.DEVNULL)
    path = str(tmp_path / "resources.json")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--match", "_kernel", "--json", path,
                           os.path.join(CSRC, "mm_policy_wide.o")], stdout=subprocess.DEVNULL)
    now = {r["kernel"]: r for r in json.load(open(path))}
    assert "mm::wide::policy_wide_kernel" in now and len(now) == 2  # the act kernel and the counter's bump
    for r in now.values():
        assert r["vgpr_spill"] == 0 and r["scratch_B"] == 0 and r["lds_B"] <= 160 * 1024, r
    rec = {r["kernel"]: r for r in json.load(open(os.path.join(REPO, "profiles", "policy_wide", "kernel_resources.json")))}
    assert set(rec) == set(now)
    for name in now:
        for k in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "lds_B"):
            assert now[name][k] == rec[name][k], (name, k)


def test_oracle_rollout_keeps_the_module_path():
    """DeviceRollout on an oracle env with a 512 actor: not fused (the CPU oracle refuses hidden 512), and it still rolls out
    through the module's forward + mm_sample_actions, one sampler step per policy step plus one for the bootstrap's action
    draw."""
    torch.manual_seed(0)
    env = oracle_env.OracleEnv(6, 4, env_id="merge-multi-agent-v1", config={"safety_guarantee": "none"}, seed=3, auto_reset=True)
    actor, critic = ActorNetwork(30, 512, 5), CriticNetwork(30, 5, 512)
    ro = DeviceRollout(env, actor, critic, roll_out_n_steps=5, sample_seed=21)
    assert not ro.shared and ro.fused_policy is False
    out = ro.interact()
    assert out["states"].shape == (5, 6, 4, 30) and out["actions"].shape == (5, 6, 4) and out["returns"].shape == (5, 6, 4)
    assert int(ro._sample_counter) == 5 + 1 and bool(torch.isfinite(out["returns"]).all())
    assert bool(((out["actions"] >= 0) & (out["actions"] < 5)).all())
    assert DeviceRollout(env, ActorNetwork(30, 128, 5), CriticNetwork(30, 5, 128)).fused_policy is True  # (128: as before)
    w = W.weights_of("act", actor)
    c = W.counter_tensor(0, "cpu")
    a = torch.zeros(4, dtype=torch.int32)
    rc = W.launch(oracle_env.library(), w, torch.zeros(4, 30), 4, 30, 5, 7, c, a, None, entry="mm_policy_act")
    assert rc == _cabi.MM_ERR_INVALID_ARG and W.counter_value(c) == 0


def test_input_conditions_of_the_gpu_grid():
    """For every synthetic case of the GPU file, from float64 and the numpy Philox alone: no row with a pre-activation of
    either hidden layer within KNIFE of zero once the redraw loop is done (asserted when a Case is built, and again here), no u
    within BAND of an inner CDF edge for n <= 1000, and a share of at most BAND_SHARE beyond."""
    worst, redrawn, rounds = 0.0, [], 0
    for case, keys in W.all_gpu_cases():
        assert not bool(W.knife_edges("act", case.net64, case.obs.double()).any()), case.name
        if case.n == 257:
            redrawn.append(case.redrawn)
            rounds = max(rounds, case.rounds)
        for seed, ctr in keys:
            near = case.near(seed, ctr)
            if case.n <= 1000:
                assert not near.any(), (case.name, hex(seed), hex(ctr), np.nonzero(near)[0])
            else:
                worst = max(worst, float(near.mean()))
                assert near.mean() <= W.BAND_SHARE, (case.name, hex(seed), hex(ctr))
    assert rounds < 20  # (the loop ended because no row was left, not because it ran out)
    print("rows redrawn per 257-row case: %d..%d in at most %d rounds; largest share of rows within %g of a CDF edge at "
          "n > 1000: %.3g" % (min(redrawn), max(redrawn), rounds, W.BAND, worst))


def test_n_boundaries_come_from_the_header():
    assert W.WG == 32 * W.WAVES and W.GRID == W.WG * W.MAX_GRID
    for edge in (W.TILE, W.WG, W.GRID):
        assert {edge - 1, edge, edge + 1} <= set(W.N_GRID_B)
    assert 1 in W.N_GRID_B and max(W.N_GRID_B) > 2 * W.GRID
