"""mm_policy_train / mm_policy_eval / PPOLearner without a GPU: the fixtures recorded from the reference's MAPPO.train()
(tools/gen_golden_mappo_train.py), a float64 restatement of marl/mappo.py:170-201 against them -- which validates the O(B)
S+ / S- form of the [B, B] objective with the advantages of the critic target before any kernel is trusted -- where the soft
update runs, and the binding surface."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle_env
from marl_mass_amd import _cabi as abi
from marl_mass_amd.rollout import ActorCriticNetwork, ActorNetwork, CriticNetwork
from policy_train_util import (FIXTURES, GRAD_NAMES, NAMES, fixture_nets, load_fixture, loss_and_grads, one_hot, pre_step_prefix,
                               sums_of)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _step_inputs(z, meta, a, dtype=torch.float64):
    """obs, actions, returns of agent step a, and old_logp / advantages from the recorded TARGETS (float64)."""
    obs = torch.tensor(z["states"][:, a, :], dtype=dtype)
    act = torch.tensor(z["actions"][:, a])
    ret = torch.tensor(z["returns"][:, a], dtype=dtype)
    ta, tc = fixture_nets(z, meta, "tp_", dtype)
    with torch.no_grad():
        old = ta(obs).gather(1, act.long().unsqueeze(1)).squeeze(1)
        adv = ret - tc(obs, one_hot(act, meta["n_a"], dtype)).squeeze(1)
    return obs, act, ret, old, adv


@pytest.mark.parametrize("run,t", FIXTURES)
def test_fixture_integrity(run, t):
    z, meta = load_fixture(run, t)
    assert meta["env_id"] == "merge-multi-agent-v1" and meta["shield"] == "none" and not meta["shared_network"]
    assert meta["run"] == run and meta["critic_loss"] == ("huber" if run == "huber" else "mse") and meta["hidden"] == 128
    assert meta["train_index"] == t and meta["clip_param"] == 0.2 and meta["optimizer_type"] == "rmsprop"
    assert meta["actor_lr"] == 1e-4 and meta["critic_lr"] == 1e-4 and meta["max_grad_norm"] == 0.5 and meta["param_names"] == NAMES
    assert (meta["target_update_steps"], meta["target_tau"]) == ((2, 0.5) if run == "soft" else (5, 1.0))
    B, N, S, A = meta["batch"], meta["n_agents"], meta["n_s"], meta["n_a"]
    assert B == (90, 70)[t] and N == 3 and meta["agent_steps"] == N and 25 <= S <= 32 and 1 <= A <= 8
    assert z["states"].shape == (B, N, S) and z["actions"].shape == (B, N) and z["returns"].shape == (B, N)
    assert z["actions"].dtype == np.int32 and 0 <= z["actions"].min() and z["actions"].max() < A
    soft = meta["n_episodes"] % meta["target_update_steps"] == 0 and meta["n_episodes"] > 0
    assert soft == (run == "soft" and t == 1) and soft == meta["soft_update_after_train"]
    shapes = {"actor." + k: tuple(v.shape) for k, v in ActorNetwork(S, 128, A).named_parameters()}
    shapes.update({"critic." + k: tuple(v.shape) for k, v in CriticNetwork(S, A, 128, 1).named_parameters()})
    assert shapes["critic.fc2.weight"] == (128, 128 + A)  # the one-hot block is part of the feature
    for k in GRAD_NAMES:
        assert z["p_" + k].shape == shapes[k] and z["tp_" + k].shape == shapes[k]
        assert ("after_tp_" + k in z) == soft
        for a in range(N):
            assert z["a%d_g_%s" % (a, k)].shape == shapes[k] and z["a%d_q_%s" % (a, k)].shape == shapes[k]
            assert np.isfinite(z["a%d_g_%s" % (a, k)]).all()
    for a in range(N):
        assert list(z["a%d_min_shape" % a]) == [B, B]  # the reference's th.min ran on the [B, B] broadcast
        assert z["a%d_losses" % a].shape == (2,)
        assert np.abs(z["a%d_g_critic.fc2.weight" % a][:, 128:]).max() > 0  # the one-hot columns have a gradient
    fresh = all(np.array_equal(z["p_" + k], z["tp_" + k]) for k in GRAD_NAMES)
    assert fresh == (t == 0)
    # ratio = 1 only on agent step 0 of train 0; and the recorded runs never reach a clip edge (synthetic batches cover it)
    for a in range(N):
        obs, act, ret, old, _ = _step_inputs(z, meta, a)
        actor = fixture_nets(z, meta, pre_step_prefix(a), torch.float64)[0]
        with torch.no_grad():
            r = torch.exp(actor(obs).gather(1, act.long().unsqueeze(1)).squeeze(1) - old)
        dev1 = float((r - 1).abs().max())
        assert dev1 == 0.0 if (t == 0 and a == 0) else dev1 > 1e-4
        assert 0.8 < float(r.min()) and float(r.max()) < 1.2


@pytest.mark.parametrize("run,t", FIXTURES)
def test_float64_restatement_reproduces_the_recorded_run(run, t):
    """The literal [B, B] expression AND its O(B) form, in float64, with advantages from the recorded critic target, against
    the reference's float32 losses and pre-clip gradients: <= 1e-5 of each tensor's max-abs."""
    z, meta = load_fixture(run, t)
    for a in range(meta["n_agents"]):
        actor, critic = fixture_nets(z, meta, pre_step_prefix(a), torch.float64)
        obs, act, ret, old, adv = _step_inputs(z, meta, a)
        for form in ("literal", "reference"):
            l2, grads = loss_and_grads(actor, critic, obs, act, ret, old, meta["clip_param"], meta["critic_loss"], form,
                                       advantages=adv, adv_sums=sums_of(adv))
            rec = z["a%d_losses" % a].astype(np.float64)
            assert np.abs(l2.numpy() - rec).max() <= 1e-5 * np.abs(rec).max(), (form, a)
            for k, g in zip(GRAD_NAMES, grads):
                r = z["a%d_g_%s" % (a, k)].astype(np.float64)
                assert np.abs(g.numpy() - r).max() <= 1e-5 * np.abs(r).max(), (form, a, k)


def test_soft_update_runs_once_after_the_agent_loop():
    """The recorded targets after train 1 of the "soft" run are (1 - tau) t + tau s applied ONCE to the final networks -- not
    once per agent step as MAPPO_GI does."""
    z, meta = load_fixture("soft", 1)
    tau, N = meta["target_tau"], meta["n_agents"]
    assert tau == 0.5
    for k in GRAD_NAMES:
        t0 = z["tp_" + k].astype(np.float64)
        final = z["a%d_q_%s" % (N - 1, k)].astype(np.float64)
        once = (1.0 - tau) * t0 + tau * final
        per_step = t0
        for a in range(N):
            per_step = (1.0 - tau) * per_step + tau * z["a%d_q_%s" % (a, k)].astype(np.float64)
        rec = z["after_tp_" + k].astype(np.float64)
        scale = max(np.abs(final - t0).max(), 1e-30)
        assert np.abs(rec - once).max() <= 2e-7 * max(1.0, np.abs(once).max())  # float32 rounding of the blend
        assert np.abs(rec - per_step).max() > 1e-2 * scale, k  # the per-step blend lands elsewhere
        assert np.abs(rec - final).max() > 1e-2 * scale and np.abs(rec - t0).max() > 1e-2 * scale  # equals neither network


def test_binding_surface():
    ora = oracle_env.library()
    assert not ora.has_policy_train  # the oracle has no twin of mm_policy_train / mm_policy_eval
    with pytest.raises(NotImplementedError):
        ora.require_policy_train()
    with pytest.raises(NotImplementedError):
        ora.policy_train_scratch_bytes(64)
    from marl_mass_amd import hip_library
    hip = hip_library()  # loading the library needs no GPU
    assert hip.has_policy_train and hasattr(hip.lib, "mm_policy_eval") and hasattr(hip.lib, "mm_policy_train_scratch_bytes")
    hip.require_policy_train()
    assert "mm_policy_train" not in abi.CLib.SYMBOLS and "mm_policy_eval" not in abi.CLib.SYMBOLS
    assert [f[0] for f in abi.MMMlpParams._fields_] == list(abi.MLP_PARAMS) == ["W1", "b1", "W2", "b2", "W3", "b3"]
    assert abi.PT_CRITIC_LOSS == {"mse": 0, "huber": 1}
    # the scratch query is host arithmetic: activations + gradients per sample, the partial blocks, monotone in n
    b0, b1, b2 = (hip.policy_train_scratch_bytes(n) for n in (0, 1000, 524288))
    assert 0 < b0 < b1 < b2 and b2 >= 524288 * 2240 and b2 - b0 <= 524288 * 2240 + 56 * 2 ** 20
    with pytest.raises(ValueError):
        hip.policy_train_scratch_bytes(-1)


def test_learner_refuses_other_networks():
    from marl_mass_amd import hip_library
    from marl_mass_amd.learner import PPOLearner
    hip = hip_library()
    ok_a, ok_c = ActorNetwork(30, 128, 5), CriticNetwork(30, 5, 128, 1)
    bad = [(ActorNetwork(30, 64, 5), CriticNetwork(30, 5, 64, 1)),        # hidden 64
           (ActorNetwork(30, 128, 5), CriticNetwork(30, 4, 128, 1)),      # different action counts
           (ActorNetwork(30, 128, 5), CriticNetwork(28, 5, 128, 1)),      # different state sizes
           (ActorNetwork(30, 128, 5), CriticNetwork(30, 5, 128, 2)),      # two critic outputs
           (ActorNetwork(30, 128, 9), CriticNetwork(30, 9, 128, 1)),      # 9 actions
           (ActorNetwork(24, 128, 5), CriticNetwork(24, 5, 128, 1)),      # 24 state columns
           (ok_a.double(), ok_c.double()),                                # float64
           (ActorNetwork(30, 128, 5), CriticNetwork(30, 5, 128, 1)),      # float32 but not on the device
           (ActorCriticNetwork(30, 5, 128, 1, state_split=True), ok_c),   # another module
           (ok_a, torch.nn.Linear(30, 1))]
    for actor, critic in bad:
        with pytest.raises(ValueError):
            PPOLearner(actor, critic, hip)
    with pytest.raises(NotImplementedError):  # the oracle cannot serve it (checked before anything is built)
        oracle_env.library().require_policy_train()


def test_kernel_resources(tmp_path):
    """The GI kernels are not touched by this translation unit -- policy_gi_kernel and the four kernels of
    mm_policy_gi_train.o are exactly as recorded -- and no new kernel spills: zero VGPR spills, zero scratch, and what
    profiles/policy_train/kernel_resources.json records is what the build gives."""
    csrc = os.path.join(REPO, "marl-mass_amd", "csrc")
    objs = ["mm_policy_gi.o", "mm_policy_gi_train.o", "mm_policy_train.o"]
    subprocess.check_call(["make", "-C", csrc] + objs, stdout=subprocess.DEVNULL)
    path = str(tmp_path / "resources.json")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--match", "_kernel", "--json", path]
                          + [os.path.join(csrc, o) for o in objs], stdout=subprocess.DEVNULL)
    rows = json.load(open(path))
    keys = ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "lds_B")
    for prof, obj, count in (("policy_gi", "mm_policy_gi.o", 1), ("policy_gi_train", "mm_policy_gi_train.o", 4)):
        rec = {r["kernel"]: r for r in json.load(open(os.path.join(REPO, "profiles", prof, "kernel_resources.json")))
               if r["object"] == obj}
        now = {r["kernel"]: r for r in rows if r["object"] == obj and (count > 1 or r["kernel"] == "mm::gi::policy_gi_kernel")}
        assert len(now) == count and set(now) <= set(rec), (obj, sorted(now))
        for name in now:
            for k in keys:
                assert now[name][k] == rec[name][k], (name, k)
    new = {r["kernel"]: r for r in rows if r["object"] == "mm_policy_train.o"}
    assert len(new) == 8  # prep, fold, sample x {actor, critic} x {train, eval}, wgrad x {actor, critic}
    for r in new.values():
        assert r["vgpr_spill"] == 0 and r["scratch_B"] == 0, r
        assert r["lds_B"] <= 160 * 1024
    rec = {r["kernel"]: r for r in json.load(open(os.path.join(REPO, "profiles", "policy_train", "kernel_resources.json")))}
    assert set(rec) == set(new)
    for name in new:
        for k in keys:
            assert new[name][k] == rec[name][k], (name, k)
