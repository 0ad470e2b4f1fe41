"""MAPPO_GI's shared actor-critic on the host: rollout.ActorCriticNetwork against the reference's recorded checkpoint
(tests/golden/mappo_gi_*.npz, tools/gen_mappo_gi_dropin.py) and DeviceRollout's shared mode on the CPU oracle."""
import json
import os

import numpy as np
import pytest
import torch

import oracle_env
from golden_util import GOLDEN
from marl_mass_amd import _cabi
from marl_mass_amd.rollout import ActorCriticNetwork, ActorNetwork, DeviceRollout

CASES = ["v1mass", "v1none", "v0prio"]
KEYS = {"fc11.weight", "fc11.bias", "fc12.weight", "fc12.bias", "fc13.weight", "fc13.bias", "fc2.weight", "fc2.bias",
        "actor_linear.weight", "actor_linear.bias", "critic_linear.weight", "critic_linear.bias"}


def _load(tag):
    z = np.load(os.path.join(GOLDEN, "mappo_gi_%s.npz" % tag))
    return z, json.loads(str(z["meta"])), json.loads(str(z["ext"]))


def _policy(z, meta):
    net = ActorCriticNetwork(meta["n_s"], meta["n_a"], 128, 1, state_split=True)
    net.load_state_dict({k[2:]: torch.tensor(z[k]) for k in z.files if k.startswith("w_")})
    return net


def _reference_split(state):
    """Model_gi.py:170-199, verbatim."""
    s1 = torch.cat([state[:, 0:1], state[:, 5:6], state[:, 10:11], state[:, 15:16], state[:, 20:21]], 1)
    s2 = torch.cat([state[:, 1:3], state[:, 6:8], state[:, 11:13], state[:, 16:18], state[:, 21:23]], 1)
    s3 = torch.cat([state[:, 3:5], state[:, 8:10], state[:, 13:15], state[:, 18:20], state[:, 23:25]], 1)
    return s1, s2, s3


def test_checkpoint_keys_load():
    """MAPPO_GI.save stores policy.state_dict(): the same names load strictly, and nothing else is in the module's."""
    z, meta, _ = _load("v1mass")
    assert {k[2:] for k in z.files if k.startswith("w_")} == KEYS
    net = ActorCriticNetwork(meta["n_s"], meta["n_a"], 128, 1, state_split=True)
    assert set(net.state_dict()) == KEYS
    net.load_state_dict({"model_state_dict": {k[2:]: torch.tensor(z[k]) for k in z.files if k.startswith("w_")}}["model_state_dict"])
    assert torch.equal(net.fc2.weight, torch.tensor(z["w_fc2.weight"]))
    assert tuple(net.fc2.weight.shape) == (128, 160) and tuple(net.fc11.weight.shape) == (32, 5)


@pytest.mark.parametrize("tag", CASES)
def test_logprobs_and_values_match_reference_checkpoint(tag):
    z, meta, _ = _load(tag)
    net = _policy(z, meta)
    for k in range(meta["K"]):
        st = torch.tensor(z["ro%d_states" % k], dtype=torch.float32).reshape(-1, meta["n_s"])
        with torch.no_grad():
            lp, v = net(st).numpy(), net(st, out_type="v").numpy()[:, 0]
        np.testing.assert_allclose(lp, z["ro%d_logp" % k].reshape(lp.shape), rtol=0, atol=2e-5)
        np.testing.assert_allclose(v, z["ro%d_value" % k].reshape(-1), rtol=0, atol=2e-5)


@pytest.mark.parametrize("n_s", [25, 30])
def test_split_gather_equals_slicing(n_s):
    torch.manual_seed(n_s)
    net = ActorCriticNetwork(n_s, 5, 128, 1, state_split=True)
    state = torch.randn(17, n_s)
    for a, b in zip(net.split(state), _reference_split(state)):
        assert torch.equal(a, b)
    # columns 25.. are never read: changing them changes nothing (the reference's quirk on 6-column rows)
    if n_s > 25:
        other = state.clone()
        other[:, 25:] = 1e6
        with torch.no_grad():
            assert torch.equal(net(state), net(other)) and torch.equal(net(state, out_type="v"), net(other, out_type="v"))


def test_forward_branches():
    """Model_gi.py:205-216: masked logits are -1e8 then log_softmax(logits + 1e-8); unmasked plain log_softmax; the
    critic head for any other out_type; and the state_split=False trunk."""
    torch.manual_seed(7)
    for split in (True, False):
        net = ActorCriticNetwork(30, 5, 128, 1, state_split=split)
        state = torch.randn(9, 30)
        mask = (torch.rand(9, 5) > 0.4).int()
        mask[:, 2] = 1
        with torch.no_grad():
            s1, s2, s3 = _reference_split(state)
            if split:
                h = torch.cat([torch.relu(net.fc11(s1)), torch.relu(net.fc12(s2)), torch.relu(net.fc13(s3))], 1)
            else:
                h = torch.relu(net.fc1(state))
            h = torch.relu(net.fc2(h))
            logits = net.actor_linear(h)
            assert torch.equal(net(state), torch.log_softmax(logits, dim=1))
            masked = logits.clone()
            masked[mask == 0] = torch.tensor([-1e8])
            assert torch.equal(net(state, action_mask=mask), torch.log_softmax(masked + 1e-8, dim=1))
            assert torch.equal(net(state, out_type="v"), net.critic_linear(h))
    assert "fc1.weight" in ActorCriticNetwork(30, 5, 128).state_dict()


def _rollout(gamma, T=9, seed=3):
    torch.manual_seed(0)
    env = oracle_env.OracleEnv(6, 4, env_id="merge-multi-agent-v1", config={"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5},
                               cbf_eta=0.03125, qp_solver="exact", cbf_tau=0.5, seed=seed, auto_reset=True)
    net = ActorCriticNetwork(30, 5, 128, 1, state_split=True)
    return DeviceRollout(env, net, roll_out_n_steps=T, reward_gamma=gamma, sample_seed=21), net


def test_shared_rollout_on_oracle_backend():
    """Shared mode on the CPU oracle (the module's forward + mm_sample_actions): shapes, one sampler step per policy step
    plus one for the bootstrap's action draw, and a bootstrap that is policy(final_obs, out_type="v")."""
    ro, net = _rollout(0.99)
    assert ro.shared and ro.critic is None and not ro.fused_policy  # the fused entry is a HIP-library one
    out = ro.interact()
    E, N, T = 6, 4, 9
    assert out["states"].shape == (T, E, N, 30) and out["actions"].shape == (T, E, N) and out["returns"].shape == (T, E, N)
    assert int(ro._sample_counter) == T + 1
    ro0, _ = _rollout(0.0)  # same stream, gamma 0: returns are the scaled rewards alone
    out0 = ro0.interact()
    assert torch.equal(out["actions"], out0["actions"]) and torch.equal(out["states"], out0["states"])
    with torch.no_grad():
        v = net(ro.obs.reshape(E * N, 30).float(), out_type="v").view(E, N).double()
    fv = (out["returns"][-1] - out0["returns"][-1]) / 0.99
    live = ~out["dones"][-1].bool()
    assert bool(live.any())
    torch.testing.assert_close(fv[live], v[live], rtol=0, atol=1e-12)
    assert bool((fv[~live] == 0).all())


def test_shared_mode_arguments():
    env = oracle_env.OracleEnv(2, 4, env_id="merge-multi-agent-v1", config={"safety_guarantee": "none"}, seed=3, auto_reset=True)
    net = ActorCriticNetwork(30, 5, 128, 1, state_split=True)
    assert DeviceRollout(env, net, net, roll_out_n_steps=2).shared
    with pytest.raises(ValueError):
        DeviceRollout(env, net, ActorCriticNetwork(30, 5, 128, 1, state_split=True))
    assert not DeviceRollout(env, ActorNetwork(30, 128, 5)).shared
    assert not oracle_env.library().has_policy_gi  # the oracle has no twin of mm_policy_gi_act


def test_hip_library_exports_policy_gi():
    """libmm_hip.so binds mm_policy_gi_act as an optional symbol, outside include/mm_abi.h's list."""
    lib = os.path.join(os.path.dirname(GOLDEN), "..", "marl-mass_amd", "csrc", "libmm_hip.so")
    import ctypes
    assert hasattr(ctypes.CDLL(lib), "mm_policy_gi_act")
    assert "mm_policy_gi_act" not in _cabi.CLib.SYMBOLS


@pytest.mark.parametrize("tag", CASES)
def test_fixture_integrity(tag):
    path = os.path.join(GOLDEN, "mappo_gi_%s.npz" % tag)
    assert os.path.getsize(path) <= 500 * 1024
    z, meta, ext = _load(tag)
    assert meta["state_split"] and meta["hidden"] == 128 and meta["K"] == 6 and meta["roll_out_n_steps"] == 40
    assert meta["test_seeds"] == [0, 25, 50] and len(ext["steps"]) == 3
    if tag == "v0prio":
        assert not meta["dropin_checked"] and meta["dropin_vs_reference_max_abs"] is None and "oracle" in meta["note"]
        assert meta["env_id"] == "merge-multi-agent-v0" and meta["shield"] == "priority"
    else:
        assert meta["dropin_checked"] and meta["dropin_vs_reference_max_abs"] <= 1e-9
        assert meta["env_id"] == "merge-multi-agent-v1" and meta["n_s"] == 30
    for k in range(meta["K"]):
        st, ac, ret = z["ro%d_states" % k], z["ro%d_actions" % k], z["ro%d_returns" % k]
        lp, v = z["ro%d_logp" % k], z["ro%d_value" % k]
        assert st.shape[:2] == ac.shape == ret.shape == lp.shape[:2] == v.shape and st.shape[2] == meta["n_s"]
        assert ((ac >= 0) & (ac < meta["n_a"])).all() and np.isfinite(ret).all() and np.isfinite(v).all()
        np.testing.assert_allclose(np.exp(lp.astype(np.float64)).sum(-1), 1.0, atol=1e-5)
    for i, s in enumerate(ext["steps"]):
        assert z["ev%d_rewards" % i].shape == (int(s),)
