"""Per-env cbf_eta / cbf_tau / HEADWAY_TIME on the device (include/mm_env_params.h, the PENV instantiations of the step
kernel): a batch whose envs carry five different parameter sets against the CPU oracle and against the uniform kernels, bit
for bit; the planes as the only source of the three values; the plumbing around them; the refusals."""
import os

import pytest
import torch

import env_params_util as U
from golden_util import episode_files, free_run, load_episode
from marl_mass_amd import VecMergeEnv, _cabi as abi
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork, DeviceRollout

pytestmark = pytest.mark.gpu


def _mixed(case, **over):
    return VecMergeEnv(U.E, case[0], env_params=U.planes(), **U.env_kw(case, **over))


_GPU_MIXED = {}


def _gpu_mixed_run(case):
    """The mixed batch's records on the GPU, once per case (the oracle and the uniform-kernel tests read the same run)."""
    if case not in _GPU_MIXED:
        env = _mixed(case)
        _GPU_MIXED[case] = U.run(env, U.tape(case[0]))
        env.poll_errors()
        env.close()
    return _GPU_MIXED[case]


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_mixed_batch_bit_exact_vs_oracle(case):
    """Env e carries set e % 5: its state planes, counters, obs, reward, agents_rewards, regional_rewards and done equal, at
    every one of 40 steps, those of the oracle run whose config carries that set (oracle_runs checks that the sets differ)."""
    want = U.oracle_runs(case)
    if case[0] >= 6:
        # set 1 (eta = 0.5) ends episodes, 2 to 8 in its uniform run of 40 envs; of those, the mixed batch meets the ones of
        # group 1's own 8 envs (one each at N = 12 and N = 11): a re-spawn under per-env values
        assert 2 <= U.dones(want[1]) <= 8
        if case[0] >= 11:
            assert U.dones(want[1], torch.nonzero(U.group_of() == 1).flatten()) >= 1
    U.assert_groups(_gpu_mixed_run(case), want, U.case_id(case))


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_mixed_batch_equals_uniform_kernels(case):
    """The same batch against five uniform-config runs of the kernels without planes, group by group; and a batch whose planes
    all hold the config's values against the run without planes."""
    N = case[0]
    uniform = []
    for s in U.SETS:
        env = VecMergeEnv(U.E, N, **U.env_kw(case, s))
        uniform.append(U.run(env, U.tape(N)))
        env.close()
    U.assert_groups(_gpu_mixed_run(case), uniform, U.case_id(case))
    for j in (0, 3):
        env = VecMergeEnv(U.E, N, env_params={}, **U.env_kw(case, U.SETS[j]))  # every key filled from the config
        assert torch.equal(env.env_params.cpu(), torch.tensor(U.SETS[j], dtype=torch.float64)[:, None].expand(3, U.E))
        got = U.run(env, U.tape(N))
        env.close()
        for t, rec in enumerate(got):
            U.assert_same(rec, uniform[j][t], (U.case_id(case), "planes == config", j, t))


def test_mixed_batch_literal_sweep():
    """debug_flags bit0 (the literal front-to-back sweep as the validation form) under per-env values: the oracle's bits."""
    case = U.CASES[0]
    env = _mixed(case, debug_flags=1)
    got = U.run(env, U.tape(case[0]))
    env.close()
    U.assert_groups(got, U.oracle_runs(case), "debug_flags=1")


def _shielded_sc_tapes():
    return [p for p in episode_files("sc_*.npz") if load_episode(p)[1]["shield"] != "none"]


def _wrong_uniform_env(E, N, **kw):
    """golden_util's constructor arguments with the tape's three values moved into the planes and deliberately wrong
    uniform values in their place; no trace."""
    kw = dict(kw)
    kw.pop("trace", None)
    cfg = dict(kw["config"])
    true = {"cbf_eta": kw["cbf_eta"], "cbf_tau": kw["cbf_tau"], "HEADWAY_TIME": cfg["HEADWAY_TIME"]}
    kw["cbf_eta"], kw["cbf_tau"], cfg["HEADWAY_TIME"] = U.WRONG
    kw["config"] = cfg
    return VecMergeEnv(E, N, env_params=true, **kw)


@pytest.mark.parametrize("path", _shielded_sc_tapes(), ids=lambda p: os.path.basename(p)[:-4])
def test_planes_are_what_is_read(path):
    """The reference's shielded crash scenarios, free-running, on an env whose CONFIG holds wrong eta / tau / HEADWAY_TIME
    and whose planes hold the tape's: steps and crash as the tape records them.  (golden_util.replay reads env.trace, which
    does not exist under planes: not run.)"""
    _, meta = load_episode(path)
    steps, crashed, mh = free_run(_wrong_uniform_env, path)
    assert (steps, crashed) == (meta["steps"], meta["crashed"])
    assert mh > 0.0


def test_wrong_uniform_values_change_the_run():
    """... and the wrong values are not harmless: a batch that carries them, in the config and in planes filled from it, gives
    other bits than set 0 (so the test above cannot pass on a kernel that reads the config)."""
    case = U.CASES[0]
    N = case[0]
    a = VecMergeEnv(U.E, N, env_params={}, **U.env_kw(case, U.WRONG))
    ra = U.run(a, U.tape(N)[:10])
    a.close()
    want = U.oracle_runs(case)[0][:10]
    assert U.envs_that_differ(ra, want, torch.arange(U.E)) >= U.E // 2


def test_in_place_update_takes_effect_at_the_next_step():
    """Writing into env.env_params between steps: the batch runs 10 steps as set 0 everywhere, then the planes are overwritten
    with the mixed sets -- the continuation equals a twin that carried set 0 in its CONFIG for 10 steps, then got the planes."""
    case = U.CASES[0]
    N, tape = case[0], U.tape(case[0])
    env = VecMergeEnv(U.E, N, env_params={}, **U.env_kw(case, U.SETS[0]))
    U.run(env, tape[:10])
    for p, k in enumerate(U.KEYS):
        env.env_params[p] = U.planes()[k].to(env.device)
    got = U.run(env, tape[10:20], fresh=False)
    twin = VecMergeEnv(U.E, N, **U.env_kw(case, U.SETS[0]))
    U.run(twin, tape[:10])
    twin.set_env_params(**U.planes())
    want = U.run(twin, tape[10:20], fresh=False)
    for t in range(10):
        U.assert_same(got[t], want[t], ("in-place update", t))
    # the update mattered: the continuation under set 0 everywhere (the oracle's) differs on the envs of the other sets
    plain = U.oracle_runs(case)[0][10:20]
    assert U.envs_that_differ(got, plain, torch.nonzero(U.group_of() != 0).flatten()) >= 8
    env.close(); twin.close()


def test_state_dict_round_trip_and_clear():
    """state_dict() carries the planes: a fresh env built WITHOUT them resumes the mixed batch bit-identically; a dict without
    the key leaves an env's planes alone; clear_env_params() returns to the config's values."""
    case = U.CASES[2]  # N = 8, ipm, HDVs
    N, tape = case[0], U.tape(case[0])
    env = _mixed(case)
    U.run(env, tape[:8])
    snap = env.state_dict()
    assert torch.equal(snap["env_params"].cpu(), env.env_params.cpu())
    want = U.run(env, tape[8:16], fresh=False)
    other = VecMergeEnv(U.E, N, **U.env_kw(case))
    assert other.env_params is None and "env_params" not in other.state_dict()
    other.load_state_dict(snap)
    got = U.run(other, tape[8:16], fresh=False)
    for t in range(8):
        U.assert_same(got[t], want[t], ("resume", t))
    old = {k: v for k, v in snap.items() if k != "env_params"}
    other.load_state_dict(old)
    assert other.env_params is not None
    other.configure(auto_reset=True)  # mm_set_config keeps the planes
    got = U.run(other, tape[8:16], fresh=False)
    for t in range(8):
        U.assert_same(got[t], want[t], ("resume from a dict without the key, after configure()", t))
    other.clear_env_params()
    assert other.env_params is None
    other.load_state_dict(old)
    cleared = U.run(other, tape[8:16], fresh=False)
    plain = VecMergeEnv(U.E, N, **U.env_kw(case))
    plain.load_state_dict(old)
    want_plain = U.run(plain, tape[8:16], fresh=False)
    for t in range(8):
        U.assert_same(cleared[t], want_plain[t], ("cleared", t))
    env.close(); other.close(); plain.close()


@pytest.mark.parametrize("case", (U.CASES[0], U.CASES[1]), ids=U.case_id)
def test_two_shards_equal_the_whole_batch(case):
    """first_env = 0, E = 24 and first_env = 24, E = 16 with the planes sliced accordingly: the whole batch's bits."""
    N, tape = case[0], U.tape(case[0])[:20]
    whole = _gpu_mixed_run(case)[:20]
    for first, count in ((0, 24), (24, 16)):
        env = VecMergeEnv(count, N, first_env=first, env_params=U.planes(count, first), **U.env_kw(case))
        got = U.run(env, [a[first:first + count] for a in tape])
        env.close()
        idx = torch.arange(first, first + count)
        for t in range(20):
            U.assert_same(got[t], whole[t], ("shard", first, t), None, idx)


def test_captured_rollout_graph_equals_eager():
    """DeviceRollout(use_graph=True), E = 16, N = 4, T = 4, on a mixed batch: the eager rollout's bits; and a graph replay sees
    planes rewritten after the capture."""
    N, En, case = 4, 16, U.CASES[0]
    torch.manual_seed(5)
    actor, critic = ActorNetwork(30, 128, 5).cuda(), CriticNetwork(30, 5, 128).cuda()
    ee = VecMergeEnv(En, N, env_params=U.planes(En), **U.env_kw(case))
    ge = VecMergeEnv(En, N, env_params=U.planes(En), **U.env_kw(case))
    eager = DeviceRollout(ee, actor, critic, roll_out_n_steps=4, sample_seed=4)
    graph = DeviceRollout(ge, actor, critic, roll_out_n_steps=4, sample_seed=4, use_graph=True)
    graph.interact()  # warm-up + capture + first replay = 2 rollouts
    eager.interact(); eager.interact()
    for it in range(4):
        if it == 2:  # rewrite the planes between rollouts: the captured graph reads the new values
            for env in (ee, ge):
                env.env_params[0].fill_(0.5)
                env.env_params[2].fill_(2.5)
        a, b = eager.interact(), graph.interact()
        torch.cuda.synchronize()
        for k in ("states", "actions", "returns", "dones", "average_speed", "min_headway"):
            assert torch.equal(a[k], b[k]), (it, k)
        assert torch.equal(ee.state.cpu(), ge.state.cpu()), it
    ee.poll_errors(); ge.poll_errors()
    ee.close(); ge.close()


def test_planes_padding_and_canary_untouched():
    """The kernels only read the planes: after 40 steps of the 12-lane layout (N = 11 of 12 slots, E = 40: tail lanes and a
    last, partly filled wave) the planes hold what was put there, the guard doubles behind them their NaN pattern, and the
    state rows of absent vehicles what the run without planes leaves there (covered by the state comparison above)."""
    case = U.CASES[5]
    env = _mixed(case)
    before = env._env_params_raw.clone()
    U.run(env, U.tape(case[0]))
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int64), env._env_params_raw.view(torch.int64))
    assert bool(torch.isnan(env._env_params_raw[3 * U.E:]).all()) and env._env_params_raw.numel() == 3 * U.E + env._ENVP_GUARD
    env.close()


def test_refusals():
    """Every refusal of include/mm_env_params.h, each with its reason in the message and never a fall-back."""
    v1 = {"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}
    p = {"cbf_eta": 0.1}
    VecMergeEnv(4, 4, env_params=p, config=v1).close()
    # the C entry on a handle outside the scope (the Python validation aside)
    for kw in (dict(env_id="merge-multi-agent-v0"), dict(env_id="merge-multi-agent-v1", config={"safety_guarantee": "none"}),
               dict(env_id="merge-multi-agent-hdv-v1")):
        env = VecMergeEnv(4, 4, **kw)
        buf = torch.zeros(3, 4, dtype=torch.float64, device=env.device)
        lib = env.clib.lib
        assert lib.mm_set_env_params(env._h, buf.data_ptr()) == abi.MM_ERR_INVALID_ARG
        assert b"mm_set_env_params" in lib.mm_last_error(env._h)
        assert lib.mm_set_env_params(env._h, None) == abi.MM_OK  # (off is always accepted)
        with pytest.raises(ValueError, match="merge-multi-agent-v1"):
            env.set_env_params(**p)
        with pytest.raises(ValueError, match="merge-multi-agent-v1"):
            VecMergeEnv(4, 4, env_params=p, **kw)
        env.close()
    env = VecMergeEnv(4, 4, env_params=p, config=v1, cbf_eta=0.03125, cbf_tau=0.5, qp_solver="exact")
    env.reset()
    # mm_set_config to a configuration outside the scope while the planes are set
    with pytest.raises(ValueError, match="per-env parameters are set"):
        env.configure(config={"safety_guarantee": "none"})
    env.config["safety_guarantee"] = "cbf-cav"
    env.configure()
    # mm_shield_actions
    z = torch.zeros(4, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="mm_shield_actions"):
        env.shield_actions(z, z)
    env.step(torch.ones(4, 4, dtype=torch.int32))  # (and the env still steps)
    env.close()
    # mm_step with a trace
    env = VecMergeEnv(4, 4, env_params=p, trace=True, config=v1, cbf_eta=0.03125, cbf_tau=0.5, qp_solver="exact")
    env.reset()
    with pytest.raises(ValueError, match="no trace"):
        env.step(torch.ones(4, 4, dtype=torch.int32))
    env.clear_env_params()
    env.step(torch.ones(4, 4, dtype=torch.int32))  # without planes the trace kernels run as before
    env.poll_errors()
    env.close()


def test_large_ipm_batch_runs_fused_under_planes():
    """A CAV-only interior-point batch large enough for the split step (debug_flags bit3 forces it at any size) runs the fused
    per-env kernel once planes are set: the oracle's bits, not the sweep kernel's uniform values."""
    case = U.CASES[1]  # N = 6, HSS, ipm, CAV-only
    env = _mixed(case, debug_flags=8)
    got = U.run(env, U.tape(case[0])[:15])
    env.close()
    U.assert_groups(got, [r[:15] for r in U.oracle_runs(case)], "debug_flags=8")
