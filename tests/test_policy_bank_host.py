"""The policy bank without a GPU: the header's constant, rollout.PolicyBank's stacking, DeviceRollout's bank-mode argument
checks, bank mode on the CPU oracle backend (the fallback: members' forwards + one mm_sample_actions), the host-side grid split
of mm_policy_bank_act, and the condition on the GPU tests' inputs that is checked here."""
import copy
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle_env
import policy_act_util as U
import policy_bank_util as B
from marl_mass_amd import _cabi as abi, hip_library
from marl_mass_amd.rollout import ActorCriticNetwork, ActorNetwork, CriticNetwork, DeviceRollout, PolicyBank

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V1 = dict(env_id="merge-multi-agent-v1", config={"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}, cbf_eta=0.03125,
          qp_solver="exact", cbf_tau=0.5, seed=3, auto_reset=True)


def test_header_constant_matches_cabi():
    text = open(os.path.join(REPO, "include", "mm_policy_bank.h")).read()
    assert int(re.search(r"#define MM_BANK_MAX_GROUPS (\d+)", text).group(1)) == abi.BANK_MAX_GROUPS == 64


def test_kernel_resources(tmp_path):
    """The cross-compile gate: policy_bank_kernel has no VGPR spills and no scratch, as policy_kernel at the same commit, its LDS
    leaves one workgroup per CU, and profiles/policy_bank/kernel_resources.json records what the build gives for both."""
    csrc = os.path.join(REPO, "marl-mass_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "mm_policy_bank.o", "mm_main.o"], stdout=subprocess.DEVNULL)
    path = str(tmp_path / "resources.json")
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--match", "policy_", "--json", path,
                           os.path.join(csrc, "mm_policy_bank.o"), os.path.join(csrc, "mm_main.o")], stdout=subprocess.DEVNULL)
    now = {r["kernel"]: r for r in json.load(open(path))}
    assert set(now) == {"mm::bank::policy_bank_kernel", "policy_kernel"}
    for r in now.values():
        assert r["vgpr_spill"] == 0 and r["scratch_B"] == 0 and 80 * 1024 < r["lds_B"] <= 160 * 1024, r
    rec = {r["kernel"]: r for r in json.load(open(os.path.join(REPO, "profiles", "policy_bank", "kernel_resources.json")))}
    assert set(rec) == set(now)
    for name in now:
        for k in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "lds_B"):
            assert now[name][k] == rec[name][k], (name, k)


def test_policy_bank_stacks_and_refreshes_in_place():
    members = [copy.deepcopy(B.member(30, k)) for k in range(4)]  # (copies: the test edits them)
    bank = PolicyBank(members)
    assert bank.K == 4 and (bank.hidden, bank.n_s, bank.n_a) == (128, 30, B.N_A)
    assert [tuple(t.shape) for t in bank.tensors] == [(4, 128, 30), (4, 128), (4, 128, 128), (4, 128), (4, 5, 128), (4, 5)]
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in bank.tensors)

    def agrees():
        for k, m in enumerate(members):
            for t, p in zip(bank.tensors, (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.fc3.weight, m.fc3.bias)):
                if not torch.equal(t[k], p.detach()):
                    return False
        return True

    assert agrees()
    assert torch.equal(bank.W2[0], bank.W2[2]) and not torch.equal(bank.W2[0], bank.W2[1])  # B.member: 2 is 0 again
    ptrs = [t.data_ptr() for t in bank.tensors]
    assert [getattr(bank.params, n) for n in abi.MLP_PARAMS] == ptrs
    with torch.no_grad():
        members[3].fc2.weight.mul_(1.5)
        members[1].fc3.bias.add_(0.25)
    assert not agrees()  # the stack is a copy
    bank.refresh()
    assert agrees() and [t.data_ptr() for t in bank.tensors] == ptrs


def test_policy_bank_refusals():
    with pytest.raises(ValueError, match="at least one"):
        PolicyBank([])
    one = ActorNetwork(30, 128, 5)
    with pytest.raises(ValueError, match="at most 64"):
        PolicyBank([one] * 65)
    PolicyBank([one] * 64)
    for other in (ActorNetwork(25, 128, 5), ActorNetwork(30, 512, 5), ActorNetwork(30, 128, 4)):
        with pytest.raises(ValueError, match="one shape"):
            PolicyBank([one, other])


def test_bank_mode_argument_checks():
    env = oracle_env.OracleEnv(8, 4, **V1)
    actors = [ActorNetwork(30, 128, 5) for _ in range(3)]
    critics = [CriticNetwork(30, 5, 128) for _ in range(3)]
    with pytest.raises(ValueError, match="sum to"):
        DeviceRollout(env, actors, group_envs=[3, 0, 4])
    with pytest.raises(ValueError, match="sum to"):
        DeviceRollout(env, actors, group_envs=[9, -1, 0])
    with pytest.raises(ValueError, match="one env count per member"):
        DeviceRollout(env, actors, group_envs=[3, 5])
    with pytest.raises(ValueError, match="one env count per member"):
        DeviceRollout(env, actors)
    with pytest.raises(ValueError, match="one critic per member"):
        DeviceRollout(env, actors, critics[:2], group_envs=[3, 0, 5])
    with pytest.raises(ValueError, match="one critic per member"):
        DeviceRollout(env, actors, critics[0], group_envs=[3, 0, 5])
    with pytest.raises(ValueError, match="bank mode"):
        DeviceRollout(env, actors[0], group_envs=[8])
    with pytest.raises(ValueError, match="one shape"):
        DeviceRollout(env, actors[:2] + [ActorNetwork(30, 512, 5)], group_envs=[3, 0, 5])
    ro = DeviceRollout(env, actors, critics, group_envs=[3, 0, 5], roll_out_n_steps=2)
    assert ro.bank_mode and not ro.fused_policy and ro.bank.K == 3  # the fused entry is a HIP-library one
    assert ro.group_index.tolist() == [0, 0, 0, 2, 2, 2, 2, 2]
    assert [ro.group_slice(k) for k in range(3)] == [slice(0, 3), slice(3, 3), slice(3, 8)]
    assert not oracle_env.library().has_policy_bank
    with pytest.raises(NotImplementedError, match="mm_policy_bank_act"):
        oracle_env.library().require_policy_bank()
    hip = hip_library()  # loading the library needs no GPU
    assert hip.has_policy_bank
    hip.require_policy_bank()


def test_bank_mode_on_oracle_backend_takes_the_fallback():
    """v1, E = 8, N = 4, K = 3, group_envs = [3, 0, 5], distinct members: act(obs) is mm_sample_actions applied to the
    concatenation of each member's module(obs_slice), and the counter advances by one per act.  (A list as `actor` is not
    accepted without the feature.)"""
    E, N = 8, 4
    env = oracle_env.OracleEnv(E, N, **V1)
    actors = [B.member(30, k) for k in (0, 1, 3)]
    ro = DeviceRollout(env, actors, group_envs=[3, 0, 5], roll_out_n_steps=3, sample_seed=21)
    assert not ro.fused_policy
    clib = oracle_env.library()
    obs = ro.obs
    for step in range(2):
        flat = obs.reshape(E * N, 30).float()
        with torch.no_grad():
            want_lp = torch.cat([actors[0](flat[:12]), actors[2](flat[12:])])
        want, _ = U.sample(clib, want_lp, 21, step)
        got = ro.act(obs)
        assert got.shape == (E, N) and got.dtype == torch.int32
        assert torch.equal(got.view(-1), want), step
        assert int(ro._sample_counter) == step + 1
        other, _ = U.sample(clib, torch.cat([actors[1](flat[:12]), actors[2](flat[12:])]).detach(), 21, step)
        assert step > 0 or not torch.equal(other, want)  # member 1 (the empty group's) would have drawn differently
        obs = env.step(got)[0]
    # interact(): shapes, one draw per step (no critic: no bootstrap draw), per-group critics on their slices
    out = ro.interact()
    assert out["actions"].shape == (3, E, N) and out["returns"].shape == (3, E, N) and int(ro._sample_counter) == 2 + 3
    critics = [CriticNetwork(30, 5, 128) for _ in range(3)]
    rc = DeviceRollout(oracle_env.OracleEnv(E, N, **V1), actors, critics, group_envs=[3, 0, 5], roll_out_n_steps=3, sample_seed=21,
                       reward_gamma=0.5)
    r0 = DeviceRollout(oracle_env.OracleEnv(E, N, **V1), actors, critics, group_envs=[3, 0, 5], roll_out_n_steps=3, sample_seed=21,
                       reward_gamma=0.0)
    a, z = rc.interact(), r0.interact()
    assert torch.equal(a["actions"], z["actions"]) and int(rc._sample_counter) == 3 + 1
    fv = (a["returns"][-1] - z["returns"][-1]) / 0.5  # the bootstrap value, where the last step did not end an episode
    flat = rc.obs.reshape(E * N, 30).float()
    fa, _ = U.sample(clib, torch.cat([actors[0](flat[:12]), actors[2](flat[12:])]).detach(), 21, 3)
    one_hot = torch.nn.functional.one_hot(fa.long(), 5).float()
    with torch.no_grad():
        v = torch.cat([critics[0](flat[:12], one_hot[:12]), critics[2](flat[12:], one_hot[12:])]).view(E, N).double()
    live = ~a["dones"][-1].bool()
    assert bool(live.any())
    torch.testing.assert_close(fv[live], v[live], rtol=0, atol=1e-12)


def test_shared_members_take_the_fallback():
    """ActorCriticNetwork members: no stack, the members' own forwards, each member its own critic."""
    E, N = 4, 4
    nets = [U.gi_net(30, 5, 3, seed=7 + k) for k in range(2)]
    ro = DeviceRollout(oracle_env.OracleEnv(E, N, **V1), nets, group_envs=[1, 3], roll_out_n_steps=2, sample_seed=5)
    assert ro.bank is None and ro.shared and not ro.fused_policy
    out = ro.interact()
    assert out["actions"].shape == (2, E, N) and int(ro._sample_counter) == 2 + 1
    with pytest.raises(ValueError, match="their own critics"):
        DeviceRollout(oracle_env.OracleEnv(E, N, **V1), nets, [None, None], group_envs=[1, 3])
    with pytest.raises(ValueError, match="all ActorCriticNetworks"):
        DeviceRollout(oracle_env.OracleEnv(E, N, **V1), [nets[0], ActorNetwork(30, 128, 5)], group_envs=[1, 3])
    assert isinstance(nets[0], ActorCriticNetwork)


@pytest.mark.parametrize("name", sorted(B.LAYOUTS))
def test_grid_split(name):
    """mm_policy_bank_grid (host arithmetic, no device): an empty group has no workgroup, every other at least one and never
    more than it has tile octets, the prefix is consistent and the grid is at most 256 + K."""
    sizes = B.LAYOUTS[name]
    K = len(sizes)
    bs = B.bank_grid(hip_library(), B.group_start(sizes))
    assert bs[0] == 0 and len(bs) == K + 1
    blocks = np.diff(bs)
    tiles = [(s + 31) // 32 for s in sizes]
    for k in range(K):
        assert (blocks[k] == 0) == (sizes[k] == 0), (name, k)
        assert blocks[k] <= (tiles[k] + 7) // 8, (name, k)
    assert 1 <= bs[K] <= 256 + K
    if sum((t + 7) // 8 for t in tiles) <= 256:
        assert list(blocks) == [(t + 7) // 8 for t in tiles]  # every wave at most one tile
    else:
        assert bs[K] >= 256  # the budget is used


def test_grid_split_is_proportional_and_bounded():
    lib = hip_library()
    # 64 equal groups of 8192 agents: 4 workgroups each
    assert np.diff(B.bank_grid(lib, B.group_start([8192] * 64))).tolist() == [4] * 64
    # 63 one-agent groups beside a huge one: every small group keeps its workgroup, the grid stays within 256 + K
    bs = B.bank_grid(lib, B.group_start([1] * 63 + [1 << 24]))
    assert np.diff(bs)[:63].tolist() == [1] * 63 and bs[64] <= 256 + 64 and np.diff(bs)[63] >= 192
    # two groups 3 : 1
    assert np.diff(B.bank_grid(lib, B.group_start([3 << 18, 1 << 18]))).tolist() == [192, 64]
    # refused tables
    out = (ctypes.c_int32 * 4)()
    for start in ([1, 2, 3], [0, 5, 4]):
        assert lib.lib.mm_policy_bank_grid(2, B.c_groups(start), out) == abi.MM_ERR_INVALID_ARG
    assert lib.lib.mm_policy_bank_grid(0, B.c_groups([0]), out) == abi.MM_ERR_INVALID_ARG
    assert lib.lib.mm_policy_bank_grid(65, B.c_groups([0] * 66), out) == abi.MM_ERR_INVALID_ARG


@pytest.mark.parametrize("n_s", B.NS)
def test_f64_reference_stays_inside_the_band_cap(n_s):
    """The condition on the inputs of the GPU tests' float64 action check, from the numpy Philox and the float64 networks
    alone: on the (1, 31, 33) layout the share of rows within BAND of an inner CDF edge is within BAND_SHARE (65 rows: none),
    and on every other layout too; no base row sits on a knife edge of any member (base() asserts it)."""
    for name, sizes in B.LAYOUTS.items():
        near = B.near(n_s, sizes)
        assert near.mean() <= U.BAND_SHARE, (name, int(near.sum()))
    assert not B.near(n_s, B.LAYOUTS["k3_off_tile"]).any()
    lp = B.logp64_of(n_s, B.LAYOUTS["k3_off_tile"])
    assert float(lp[1:32].max(-1).values.exp().min()) > 0.5  # member 1 (gain 60): near-deterministic rows
