"""The bank of shared actor-critics without a GPU: rollout.SharedPolicyBank's stacking, bank mode with ActorCriticNetwork members
on the CPU oracle backend (the fallback), the library flags, the cross-compile gate of mm_policy_gi_bank.o, and the condition on
the GPU tests' inputs that is checked here."""
import copy
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import oracle_env
import policy_act_util as U
import policy_gi_bank_util as G
from marl_mass_amd import _cabi as abi, hip_library
from marl_mass_amd.rollout import ActorCriticNetwork, ActorNetwork, DeviceRollout, SharedPolicyBank

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V1 = dict(env_id="merge-multi-agent-v1", config={"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}, cbf_eta=0.03125,
          qp_solver="exact", cbf_tau=0.5, seed=3, auto_reset=True)
SHAPES = [(32, 5), (32,), (64, 10), (64,), (64, 10), (64,), (128, 160), (128,), (5, 128), (5,), (1, 128), (1,)]


@pytest.mark.parametrize("n_s", G.NS)
def test_f64_reference_stays_inside_the_band_cap(n_s):
    """The condition on the inputs of the GPU tests' float64 action check, from the numpy Philox and the float64 networks
    alone: on every layout the share of rows within BAND of an inner CDF edge is within BAND_SHARE, on (1, 31, 33) there is no
    such row; no base row sits on a knife edge of any member (base() asserts it)."""
    for name, sizes in G.LAYOUTS.items():
        near = G.near(n_s, sizes)
        assert near.mean() <= U.BAND_SHARE, (name, int(near.sum()))
    assert not G.near(n_s, G.LAYOUTS["k3_off_tile"]).any()
    lp = G.logp64_of(n_s, G.LAYOUTS["k3_off_tile"])
    assert float(lp[1:32].max(-1).values.exp().min()) > 0.5  # member 1 (gain 60): near-deterministic rows


def test_shared_policy_bank_stacks_and_refreshes_in_place():
    members = [copy.deepcopy(G.member(30, k)) for k in range(4)]  # (copies: the test edits them)
    bank = SharedPolicyBank(members)
    assert bank.K == 4 and (bank.hidden, bank.n_a) == (128, G.N_A)
    assert [tuple(t.shape) for t in bank.tensors] == [(4,) + s for s in SHAPES]
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in bank.tensors)

    def agrees():
        return all(torch.equal(t[k], p) for k, m in enumerate(members) for t, p in zip(bank.tensors, U.weights_of("gi", m)))

    assert agrees()
    assert torch.equal(bank.W2[0], bank.W2[2]) and not torch.equal(bank.W2[0], bank.W2[1])  # G.member: 2 is 0 again
    ptrs = [t.data_ptr() for t in bank.tensors]
    assert isinstance(bank.params, abi.MMGiParams) and [getattr(bank.params, n) for n in abi.GI_PARAMS] == ptrs
    assert [getattr(bank, n).data_ptr() for n in abi.GI_PARAMS] == ptrs
    with torch.no_grad():
        members[3].fc2.weight.mul_(1.5)
        members[1].critic_linear.bias.add_(0.25)
        members[0].fc11.weight.add_(0.125)
    assert not agrees()  # the stack is a copy
    bank.refresh()
    assert agrees() and [t.data_ptr() for t in bank.tensors] == ptrs


def test_shared_policy_bank_refusals():
    with pytest.raises(ValueError, match="at least one"):
        SharedPolicyBank([])
    one = ActorCriticNetwork(30, 5, 128, 1, state_split=True)
    with pytest.raises(ValueError, match="at most 64"):
        SharedPolicyBank([one] * 65)
    assert SharedPolicyBank([one] * 64).K == 64
    with pytest.raises(ValueError, match="one shape"):
        SharedPolicyBank([one, ActorCriticNetwork(30, 4, 128, 1, state_split=True)])
    for other in (ActorCriticNetwork(30, 5, 128, 1, state_split=False), ActorCriticNetwork(30, 5, 256, 1, state_split=True),
                  ActorNetwork(30, 128, 5)):
        with pytest.raises(ValueError, match="state_split ActorCriticNetworks of hidden 128"):
            SharedPolicyBank([one, other])


def test_shared_members_on_the_oracle_backend_still_take_the_fallback():
    """v1, E = 4, N = 4, two distinct state-split hidden-128 members on the CPU oracle: no stack, fused_policy off, act() is
    mm_sample_actions on the members' module rows, and the bootstrap draws once more."""
    E, N = 4, 4
    nets = [G.member(30, k) for k in (0, 1)]
    ro = DeviceRollout(oracle_env.OracleEnv(E, N, **V1), nets, group_envs=[1, 3], roll_out_n_steps=2, sample_seed=5)
    assert ro.bank is None and ro.shared_bank is None and ro.shared and not ro.fused_policy
    flat = ro.obs.reshape(E * N, 30).float()
    with torch.no_grad():
        rows = torch.cat([nets[0](flat[:4]), nets[1](flat[4:])])
    want, _ = U.sample(oracle_env.library(), rows, 5, 0)
    assert torch.equal(ro.act(ro.obs).view(-1), want) and int(ro._sample_counter) == 1
    out = ro.interact()
    assert out["actions"].shape == (2, E, N) and int(ro._sample_counter) == 1 + 2 + 1


def test_library_flags():
    assert not oracle_env.library().has_policy_gi_bank
    with pytest.raises(NotImplementedError, match="mm_policy_gi_bank_act"):
        oracle_env.library().require_policy_gi_bank()
    hip = hip_library()  # loading the library needs no GPU
    assert hip.has_policy_gi_bank  # (fails without the feature)
    hip.require_policy_gi_bank()
    assert "mm_policy_gi_bank_act" not in abi.CLib.SYMBOLS  # not part of include/mm_abi.h's symbol list


def test_refusals_touch_no_device():
    """The entry refuses before it enqueues anything, so every refusal and the n = 0 call return without a GPU (the pointers
    are never dereferenced: 4096 stands for a device address)."""
    lib, p = hip_library().lib, 4096
    full = abi.MMGiParams(*[p] * 12)

    def call(obs=p, n=65, n_s=30, bank=full, K=3, start=(0, 1, 32, 65), hidden=128, n_a=5, counter=p, actions=p, logp=p, value=p):
        return lib.mm_policy_gi_bank_act(obs, n, n_s, None if bank is None else ctypes.byref(bank), K,
                                         None if start is None else G.c_groups(list(start)), hidden, n_a, 7, counter, actions, logp,
                                         value, None)

    refused = [dict(obs=None), dict(bank=None), dict(start=None), dict(K=0), dict(K=65, start=[0] * 65 + [65]), dict(hidden=512),
               dict(n_s=24), dict(n_s=33), dict(n_a=0), dict(n_a=9), dict(n=-1, start=(0, 0, 0, -1)),
               dict(actions=None, logp=None, value=None), dict(counter=None), dict(start=(1, 1, 32, 65)), dict(start=(0, 40, 32, 65)),
               dict(start=(0, 1, 32, 64)), dict(start=(0, 1, 32, 66))]
    refused += [dict(bank=abi.MMGiParams(*[None if i == j else p for i in range(12)])) for j in range(12)]
    for change in refused:
        assert call(**change) == abi.MM_ERR_INVALID_ARG, change
    assert call(n=0, start=(0, 0, 0, 0)) == abi.MM_OK


def test_kernel_resources(tmp_path):
    """The cross-compile gate: mm_policy_gi_bank.o holds policy_gi_bank_kernel and the counter bump and nothing else; the kernel
    has no VGPR spills and no scratch, its LDS (policy_gi_kernel's fragments) leaves one workgroup per CU, and
    profiles/policy_gi_bank/kernel_resources.json records what the build gives."""
    csrc = os.path.join(REPO, "marl-mass_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "mm_policy_gi_bank.o"], stdout=subprocess.DEVNULL)
    path = str(tmp_path / "resources.json")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--match", "_kernel", "--json", path,
                           os.path.join(csrc, "mm_policy_gi_bank.o")], stdout=subprocess.DEVNULL)
    now = {r["kernel"]: r for r in json.load(open(path))}
    assert set(now) == {"mm::gi_bank::policy_gi_bank_kernel", "mm::gi_bank::counter_bump_kernel"}
    r = now["mm::gi_bank::policy_gi_bank_kernel"]
    assert r["vgpr_spill"] == 0 and r["scratch_B"] == 0 and 80 * 1024 < r["lds_B"] <= 160 * 1024, r
    rec = {r["kernel"]: r for r in json.load(open(os.path.join(REPO, "profiles", "policy_gi_bank", "kernel_resources.json")))}
    assert set(rec) == set(now)
    for name in now:
        for k in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "lds_B"):
            assert now[name][k] == rec[name][k], (name, k)
