"""mm_policy_gi_train / SharedPPOLearner without a GPU: the fixtures recorded from the reference's MAPPO_GI.train()
(tools/gen_golden_gi_train.py), a float64 restatement of marl/mappo_gi.py:305-339 against them -- which validates the O(B)
S+ / S- form of the [B, B] objective on the CPU before any kernel is trusted -- and the binding surface."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle_env
from gi_train_util import FIXTURES, GRAD_NAMES, fixture_net, load_fixture, loss_and_grads
from marl_mass_amd import _cabi as abi
from marl_mass_amd.rollout import ActorCriticNetwork

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("loss,t", FIXTURES)
def test_fixture_integrity(loss, t):
    z, meta = load_fixture(loss, t)
    assert meta["env_id"] == "merge-multi-agent-v1" and meta["shield"] == "none" and meta["ini"].endswith("shared-unsafe.ini")
    assert meta["shared_network"] and meta["state_split"] and meta["hidden"] == 128 and meta["critic_loss"] == loss
    assert meta["train_index"] == t and meta["clip_param"] == 0.2 and meta["optimizer_type"] == "rmsprop" and meta["lr"] == 1e-4
    assert meta["max_grad_norm"] == 0.5 and meta["param_names"] == GRAD_NAMES
    B, N, S = meta["batch"], meta["n_agents"], meta["n_s"]
    assert 64 <= B <= 100 and 1 <= N <= 4 and meta["agent_steps"] == N
    assert z["states"].shape == (B, N, S) and z["actions"].shape == (B, N) and z["returns"].shape == (B, N)
    assert z["actions"].dtype == np.int32 and 0 <= z["actions"].min() and z["actions"].max() < meta["n_a"]
    # no soft update ran inside this train(): the target stays the initial network of train 0
    assert not (meta["n_episodes"] % meta["target_update_steps"] == 0 and meta["n_episodes"] > 0)
    net = ActorCriticNetwork(S, meta["n_a"], 128, 1, state_split=True)
    shapes = {k: tuple(v.shape) for k, v in net.named_parameters()}
    for k in GRAD_NAMES:
        assert z["p_" + k].shape == shapes[k] and z["tp_" + k].shape == shapes[k]
        for a in range(N):
            assert z["a%d_g_%s" % (a, k)].shape == shapes[k] and z["a%d_q_%s" % (a, k)].shape == shapes[k]
            assert np.isfinite(z["a%d_g_%s" % (a, k)]).all()
    for a in range(N):
        assert list(z["a%d_min_shape" % a]) == [B, B]  # the reference's th.min ran on the [B, B] broadcast
        l3 = z["a%d_losses" % a]
        assert l3.shape == (3,) and abs(float(l3[0]) + float(l3[1]) - float(l3[2])) <= 1e-6 * max(1.0, abs(float(l3[2])))
    fresh = all(np.array_equal(z["p_" + k], z["tp_" + k]) for k in GRAD_NAMES)
    assert fresh == (t == 0)  # train 0: ratio = 1 everywhere; train 1: the policy has moved, the target has not


@pytest.mark.parametrize("loss,t", FIXTURES)
def test_float64_restatement_reproduces_the_recorded_run(loss, t):
    """The literal [B, B] expression AND its O(B) form, in float64, against the reference's float32 losses and pre-clip
    gradients: <= 1e-5 of each tensor's max-abs."""
    z, meta = load_fixture(loss, t)
    target = fixture_net(z, meta, "tp_", torch.float64)
    for a in range(meta["n_agents"]):
        net = fixture_net(z, meta, "p_" if a == 0 else "a%d_q_" % (a - 1), torch.float64)
        obs = torch.tensor(z["states"][:, a, :], dtype=torch.float64)
        act = torch.tensor(z["actions"][:, a])
        ret = torch.tensor(z["returns"][:, a], dtype=torch.float64)
        with torch.no_grad():
            old = target(obs).gather(1, act.long().unsqueeze(1)).squeeze(1)
            adv = ret - net(obs, out_type="v").squeeze(1)
            sums = torch.stack([adv.clamp(min=0).sum(), adv.clamp(max=0).sum()])
            dev1 = float((torch.exp(net(obs).gather(1, act.long().unsqueeze(1)).squeeze(1) - old) - 1).abs().max())
            # ratio = 1 everywhere only on agent step 0 of train 0: every later step runs on a policy that has already moved
            assert dev1 == 0.0 if (t == 0 and a == 0) else dev1 > 1e-4
        for form in ("literal", "reference"):
            l3, grads = loss_and_grads(net, obs, act, ret, old, meta["clip_param"], loss, form, adv_sums=sums)
            rec = z["a%d_losses" % a].astype(np.float64)
            assert np.abs(l3.numpy() - rec).max() <= 1e-5 * np.abs(rec).max(), (form, a)
            for k, g in zip(GRAD_NAMES, grads):
                r = z["a%d_g_%s" % (a, k)].astype(np.float64)
                assert np.abs(g.numpy() - r).max() <= 1e-5 * np.abs(r).max(), (form, a, k)


def test_binding_surface():
    ora = oracle_env.library()
    assert not ora.has_policy_gi_train  # the oracle has no twin of mm_policy_gi_train
    with pytest.raises(NotImplementedError):
        ora.require_policy_gi_train()
    with pytest.raises(NotImplementedError):
        ora.policy_gi_train_scratch_bytes(64)
    from marl_mass_amd import hip_library
    hip = hip_library()  # loading the library needs no GPU
    assert hip.has_policy_gi_train
    hip.require_policy_gi_train()
    assert "mm_policy_gi_train" not in abi.CLib.SYMBOLS  # not part of include/mm_abi.h's list
    assert [f[0] for f in abi.MMGiParams._fields_] == list(abi.GI_PARAMS) and len(abi.GI_PARAMS) == 12
    # the scratch query is host arithmetic: activations + gradients per sample, the partial blocks, monotone in n
    b0, b1, b2 = (hip.policy_gi_train_scratch_bytes(n) for n in (0, 1000, 524288))
    assert 0 < b0 < b1 < b2 and b2 >= 524288 * (2 * 160 + 2 * 128) * 4
    with pytest.raises(ValueError):
        hip.policy_gi_train_scratch_bytes(-1)


def test_learner_refuses_other_networks():
    from marl_mass_amd import hip_library
    from marl_mass_amd.learner import SharedPPOLearner
    hip = hip_library()
    with pytest.raises(ValueError):
        SharedPPOLearner(ActorCriticNetwork(30, 5, 128, 1, state_split=False), hip)
    with pytest.raises(ValueError):
        SharedPPOLearner(ActorCriticNetwork(30, 5, 64, 1, state_split=True), hip)
    with pytest.raises(ValueError):
        SharedPPOLearner(ActorCriticNetwork(30, 5, 128, 1, state_split=True).double(), hip)
    with pytest.raises(ValueError):
        SharedPPOLearner(torch.nn.Linear(30, 5), hip)


def test_policy_gi_kernel_resources_unchanged(tmp_path):
    """mm_policy_gi_act's kernel is not touched by the training entry: registers, spills, scratch and LDS of
    policy_gi_kernel are the recorded ones (profiles/policy_gi/kernel_resources.json)."""
    csrc = os.path.join(REPO, "marl-mass_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "mm_policy_gi.o", "mm_policy_gi_train.o"], stdout=subprocess.DEVNULL)
    path = str(tmp_path / "resources.json")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--match", "_kernel", "--json", path,
                           os.path.join(csrc, "mm_policy_gi.o"), os.path.join(csrc, "mm_policy_gi_train.o")],
                          stdout=subprocess.DEVNULL)
    rows = json.load(open(path))
    rec = [r for r in json.load(open(os.path.join(REPO, "profiles", "policy_gi", "kernel_resources.json")))
           if r["kernel"] == "mm::gi::policy_gi_kernel"][0]
    now = [r for r in rows if r["kernel"] == "mm::gi::policy_gi_kernel"][0]
    for k in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "lds_B"):
        assert now[k] == rec[k], k
    # the budget of the new kernels: nothing spills to scratch memory
    new = [r for r in rows if r["object"] == "mm_policy_gi_train.o"]
    assert len(new) == 4
    for r in new:
        assert r["vgpr_spill"] == 0 and r["scratch_B"] == 0, r
