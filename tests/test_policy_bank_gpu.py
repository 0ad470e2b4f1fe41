"""mm_policy_bank_act (include/mm_policy_bank.h) and DeviceRollout's bank mode on the MI355X.

The existing single-actor entry is the reference: group k's log-probability rows are bit-equal to mm_policy_act on that slice with
member k's weights, the actions are mm_sample_actions' draws from the bank's own rows at the global agent index, and the rows
agree with the float64 module under policy_act_util.compare (the rule and the factor of the mm_policy_act tests).  Members,
layouts and the float64 reference: policy_bank_util."""
import copy

import numpy as np
import pytest
import torch

import policy_act_util as U
import policy_bank_util as B
from marl_mass_amd import VecMergeEnv, _cabi as abi, hip_library
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork, DeviceRollout, group_ext_info

pytestmark = pytest.mark.gpu

DEV = "cuda"
ERRORS = {}
V1 = dict(config={"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}, cbf_eta=0.03125, qp_solver="exact", cbf_tau=0.5, seed=9,
          auto_reset=True)
KEYS = ("states", "actions", "returns", "dones", "average_speed", "min_headway")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _members(n_s, K):
    return [copy.deepcopy(B.member(n_s, k)).to(DEV) for k in range(K)]


def _single(clib, net, obs, seed, ctr):
    """mm_policy_act on obs with one member: {actions, logp, counter}."""
    return U.run(clib, "act", U.weights_of("act", net), obs.contiguous(), B.N_A, seed, ctr)


@pytest.mark.parametrize("n_s", B.NS)
@pytest.mark.parametrize("name", sorted(B.LAYOUTS))
def test_layout(name, n_s):
    clib = hip_library()
    sizes = B.LAYOUTS[name]
    K, n, start = len(sizes), int(sum(sizes)), B.group_start(sizes)
    members = _members(n_s, K)
    tensors = B.stack(members, DEV)
    params = B.bank_params(tensors)
    obs = B.obs_of(n_s, n).to(DEV)
    # ---- 4. guarded buffers at an offset of one element
    actions, chk_a = U.guarded(n, torch.int32, DEV)
    logp, chk_l = U.guarded(n * B.N_A, torch.float32, DEV)
    ctr = U.counter_tensor(B.CTR, DEV)
    assert B.launch_bank(clib, params, obs, n, n_s, K, B.c_groups(start), B.SEED, ctr, actions, logp) == abi.MM_OK
    torch.cuda.synchronize()
    chk_a(); chk_l()
    assert U.counter_value(ctr) == B.CTR + 1
    logp = logp.view(n, B.N_A)
    assert bool(torch.isfinite(logp).all()) and bool(((actions >= 0) & (actions < B.N_A)).all())
    # the logp = NULL path: the same actions, nothing else written
    actions2, chk_a2 = U.guarded(n, torch.int32, DEV)
    ctr2 = U.counter_tensor(B.CTR, DEV)
    assert B.launch_bank(clib, params, obs, n, n_s, K, B.c_groups(start), B.SEED, ctr2, actions2, None) == abi.MM_OK
    torch.cuda.synchronize()
    chk_a2()
    assert torch.equal(actions, actions2) and U.counter_value(ctr2) == B.CTR + 1
    # ---- 1. rows of group k == mm_policy_act on the slice with member k, bit for bit
    f32 = torch.empty(n, B.N_A, device=DEV)
    for k in range(K):
        lo, hi = start[k], start[k + 1]
        if hi == lo:
            continue
        one = _single(clib, members[k], obs[lo:hi], B.SEED, B.CTR)
        assert torch.equal(_bits(logp[lo:hi]), _bits(one["logp"])), (name, k)
        if K == 1:
            assert torch.equal(actions, one["actions"]), name
        elif not torch.equal(tensors[2][k], tensors[2][(k + 1) % K]):
            wrong = _single(clib, members[(k + 1) % K], obs[lo:hi], B.SEED, B.CTR)
            assert not torch.equal(_bits(logp[lo:hi]), _bits(wrong["logp"])), (name, k)  # a wrong member cannot pass
        with torch.no_grad():
            f32[lo:hi] = members[k](obs[lo:hi])
    # ---- 2. actions == mm_sample_actions on the bank's own rows, global index; and the float64 inverse CDF outside BAND
    own, c = U.sample(clib, logp, B.SEED, B.CTR)
    assert torch.equal(actions, own) and c == B.CTR + 1
    near = B.near(n_s, sizes)
    assert near.mean() <= U.BAND_SHARE
    assert np.array_equal(actions.cpu().numpy()[~near], B.actions64(n_s, sizes)[~near]), name
    # ---- 3. the float64 module forward, under the mm_policy_act tests' rule and factor
    U.compare(ERRORS, "%s_s%d" % (name, n_s), {"logp": logp}, {"logp": f32}, {"logp": B.logp64_of(n_s, sizes)})
    assert float(torch.logsumexp(logp.double(), -1).abs().max()) <= 1e-6


def test_results_do_not_depend_on_the_split():
    """The same 65 548 rows under one member as K = 1, as (65 541, 7) and as 64 uneven groups of identical members: one set of
    bits (tile origin, workgroup count and persistent stride all differ between the three launches)."""
    clib = hip_library()
    n, n_s = 65548, 30
    obs = B.obs_of(n_s, n).to(DEV)
    net = copy.deepcopy(B.member(n_s, 0)).to(DEV)
    want = _single(clib, net, obs, B.SEED, B.CTR)
    sizes64 = [1 + 30 * k for k in range(63)]
    sizes64.append(n - sum(sizes64))
    for sizes in ((n,), (65541, 7), tuple(sizes64)):
        K = len(sizes)
        params = B.bank_params(B.stack([net] * K, DEV))
        actions = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        logp = torch.full((n, B.N_A), float("nan"), device=DEV)
        ctr = U.counter_tensor(B.CTR, DEV)
        assert B.launch_bank(clib, params, obs, n, n_s, K, B.c_groups(B.group_start(sizes)), B.SEED, ctr, actions, logp) == abi.MM_OK
        assert torch.equal(actions, want["actions"]) and torch.equal(_bits(logp), _bits(want["logp"])), K


def test_refusals():
    """Every refused call returns MM_ERR_INVALID_ARG with the outputs at their fill and the counter unchanged; n = 0 is MM_OK
    and leaves the counter alone too."""
    clib = hip_library()
    n_s, sizes = 30, (1, 31, 33)
    K, n, start = 3, 65, B.group_start((1, 31, 33))
    tensors = B.stack(_members(n_s, K), DEV)
    obs = B.obs_of(n_s, n).to(DEV)
    actions = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    logp = torch.full((n, B.N_A), float("nan"), device=DEV)
    ctr = U.counter_tensor(B.CTR, DEV)
    ok = dict(params=B.bank_params(tensors), obs=obs, n=n, n_s=n_s, K=K, start=B.c_groups(start), seed=B.SEED, counter=ctr,
              actions=actions, logp=logp, hidden=128, n_a=B.N_A)
    refused = [("obs NULL", dict(obs=None)), ("bank NULL", dict(params=None)), ("group_start NULL", dict(start=None)),
               ("counter NULL", dict(counter=None)), ("actions NULL", dict(actions=None)),
               ("K 0", dict(K=0)), ("K 65", dict(K=65, start=B.c_groups([0] * 65 + [n]))),
               ("hidden 512", dict(hidden=512)), ("hidden 64", dict(hidden=64)), ("n_s 0", dict(n_s=0)), ("n_s 33", dict(n_s=33)),
               ("n_a 0", dict(n_a=0)), ("n_a 9", dict(n_a=9)), ("n < 0", dict(n=-1, start=B.c_groups([0, 0, 0, -1]))),
               ("group_start[0] != 0", dict(start=B.c_groups([1, 1, 32, 65]))),
               ("group_start decreases", dict(start=B.c_groups([0, 40, 32, 65]))),
               ("group_start ends short of n", dict(start=B.c_groups([0, 1, 32, 64]))),
               ("group_start ends past n", dict(start=B.c_groups([0, 1, 32, 66])))]
    refused += [("member base %s NULL" % abi.MLP_PARAMS[j], dict(params=B.bank_params(tensors, null=j))) for j in range(6)]
    for what, change in refused:
        assert B.launch_bank(clib, **dict(ok, **change)) == abi.MM_ERR_INVALID_ARG, what
    assert B.launch_bank(clib, **dict(ok, n=0, start=B.c_groups([0, 0, 0, 0]))) == abi.MM_OK
    torch.cuda.synchronize()
    assert bool((actions == -7).all()) and bool(torch.isnan(logp).all()) and U.counter_value(ctr) == B.CTR
    assert B.launch_bank(clib, **ok) == abi.MM_OK  # and the well-formed call goes through
    torch.cuda.synchronize()
    assert bool((actions >= 0).all()) and U.counter_value(ctr) == B.CTR + 1


def test_graph_capture_replays_draw_fresh_numbers():
    """Two bank launches captured into one single-chain graph, replayed twice: each replay equals the eager sequence at the
    same counter values; the host group table is overwritten after the capture (the launch carries its own copy)."""
    clib = hip_library()
    n_s, sizes = 30, (1, 31, 33)
    K, n, start = 3, 65, B.group_start(sizes)
    params = B.bank_params(B.stack(_members(n_s, K), DEV))
    obs = B.obs_of(n_s, n).to(DEV)

    def eager(c0):
        ctr, outs = U.counter_tensor(c0, DEV), []
        for _ in range(4):
            a = torch.full((n,), -1, dtype=torch.int32, device=DEV)
            assert B.launch_bank(clib, params, obs, n, n_s, K, B.c_groups(start), B.SEED, ctr, a, None) == abi.MM_OK
            outs.append(a)
        torch.cuda.synchronize()
        assert U.counter_value(ctr) == c0 + 4
        return outs

    want = eager(B.CTR)
    assert not torch.equal(want[0], want[1])
    ctr = U.counter_tensor(B.CTR, DEV)
    a1 = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    a2 = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    table = B.c_groups(start)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        assert B.launch_bank(clib, params, obs, n, n_s, K, table, B.SEED, ctr, a1, None) == abi.MM_OK
        assert B.launch_bank(clib, params, obs, n, n_s, K, table, B.SEED, ctr, a2, None) == abi.MM_OK
    for k in range(K + 1):
        table[k] = 0
    assert U.counter_value(ctr) == B.CTR  # a capture runs nothing
    for r in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a1, want[2 * r]) and torch.equal(a2, want[2 * r + 1]), r
        assert U.counter_value(ctr) == B.CTR + 2 * (r + 1)


# ---- DeviceRollout's bank mode: v1 MASS, exact QP, E = 16, N = 4, T = 4, K = 4
E, N, T, K4 = 16, 4, 4, 4


def _bank_rollout(actors, critics=None, **kw):
    return DeviceRollout(VecMergeEnv(E, N, **V1), actors, critics, roll_out_n_steps=T, sample_seed=4, group_envs=[4] * K4, **kw)


@pytest.mark.parametrize("with_critic", [False, True])
def test_rollout_identical_members_equal_single_actor_twin(with_critic):
    """Four identical members: every tensor of interact() is bit-equal to a single-actor DeviceRollout twin with the same seeds.
    With critics the bootstrap value is four torch forwards on 16-row slices against the twin's one on 64 rows: the same float32
    products summed by whatever GEMM the BLAS picks for each shape, so `returns` is compared within the float32 bound of a
    133-term dot product of the critic's widest layer, 133 * 2^-24 * max|value| <= 1e-5 * max(1, max|value|); everything else
    stays bit-equal."""
    torch.manual_seed(5)
    actor = ActorNetwork(30, 128, 5).to(DEV)
    critic = CriticNetwork(30, 5, 128).to(DEV) if with_critic else None
    twin = DeviceRollout(VecMergeEnv(E, N, **V1), actor, critic, roll_out_n_steps=T, sample_seed=4)
    bank = _bank_rollout([copy.deepcopy(actor) for _ in range(K4)], [copy.deepcopy(critic) for _ in range(K4)] if with_critic else None)
    assert bank.fused_policy and twin.fused_policy and bank.bank.K == K4
    assert bank.group_index.tolist() == [k for k in range(K4) for _ in range(4)] and bank.group_slice(2) == slice(8, 12)
    for it in range(2):
        a, b = twin.interact(), bank.interact()
        torch.cuda.synchronize()
        for key in KEYS:
            if with_critic and key == "returns":
                bound = 1e-5 * max(1.0, float(a[key].abs().max()))
                assert float((a[key] - b[key]).abs().max()) <= bound, (it, key)
            else:
                assert torch.equal(a[key], b[key]), (it, key)
        assert torch.equal(twin.env.state.cpu(), bank.env.state.cpu()) and int(twin._sample_counter) == int(bank._sample_counter)
    twin.env.poll_errors(); bank.env.poll_errors()
    twin.env.close(); bank.env.close()


def test_rollout_distinct_members_act_on_their_own_groups():
    """Four distinct members: actions[t] is reproduced from states[t] by per-slice mm_policy_act rows plus ONE
    mm_sample_actions at counter value t."""
    clib = hip_library()
    actors = _members(30, K4)
    ro = _bank_rollout(actors)
    assert ro.fused_policy
    out = ro.interact()
    torch.cuda.synchronize()
    differs = 0
    for t in range(T):
        flat = out["states"][t].reshape(E * N, 30)
        rows = torch.cat([_single(clib, actors[k], flat[16 * k:16 * k + 16], 4, t)["logp"] for k in range(K4)])
        want, _ = U.sample(clib, rows, 4, t)
        assert torch.equal(out["actions"][t].view(-1), want), t
        alone = _single(clib, actors[0], flat, 4, t)["actions"]
        differs += int((alone != want).sum())
    assert differs > 0  # member 0 alone would have acted differently
    assert int(ro._sample_counter) == T  # no critic: no bootstrap draw
    # the fallback (fused_policy off: members' forwards + one mm_sample_actions) is the same stream up to float32 rows
    fb = _bank_rollout(actors, fused_policy=False)
    assert not fb.fused_policy
    assert torch.equal(fb.interact()["states"][0], out["states"][0]) and int(fb._sample_counter) == T
    ro.env.close(); fb.env.close()


def test_rollout_graph_sees_an_edited_member():
    """use_graph=True with an in-place edit of one member between two replays: the bits of an eager twin given the same edit
    (interact() refreshes the stack the captured launches read)."""
    torch.manual_seed(6)
    ea, ga = _members(30, K4), _members(30, K4)
    ec = [CriticNetwork(30, 5, 128).to(DEV) for _ in range(K4)]
    gc = [copy.deepcopy(c) for c in ec]
    eager, graph = _bank_rollout(ea, ec), _bank_rollout(ga, gc, use_graph=True)
    graph.interact()  # warm-up + capture + first replay = 2 rollouts
    eager.interact(); eager.interact()
    for it in range(3):
        if it == 1:
            with torch.no_grad():
                for nets in (ea, ga):
                    nets[2].fc3.weight.mul_(-3.0)
                    nets[2].fc1.bias.add_(0.5)
        a, b = eager.interact(), graph.interact()
        torch.cuda.synchronize()
        for key in KEYS:
            assert torch.equal(a[key], b[key]), (it, key)
        assert torch.equal(eager.env.state.cpu(), graph.env.state.cpu()), it
    # the edit reached the graph's launches: the edited member's stack rows are the new weights
    assert torch.equal(graph.bank.W3[2], ga[2].fc3.weight.detach())
    eager.env.poll_errors(); graph.env.poll_errors()
    eager.env.close(); graph.env.close()


def test_evaluate_on_a_group_major_env_params_grid():
    """K = 2 on a batch whose env_params differ per group: per-env results, two finite rows from group_ext_info, and the
    training stream restored bit for bit."""
    En = 8
    eta = torch.cat([torch.full((4,), 0.03125), torch.full((4,), 0.5)]).double()
    hw = torch.cat([torch.full((4,), 0.5), torch.full((4,), 1.2)]).double()

    def make():
        env = VecMergeEnv(En, N, env_params={"cbf_eta": eta, "HEADWAY_TIME": hw}, **V1)
        return DeviceRollout(env, _members(30, 2), roll_out_n_steps=T, sample_seed=4, group_envs=[4, 4])

    a, b = make(), make()
    assert a.fused_policy
    a.interact(); b.interact()
    before = a.env.state.clone()
    seeds = [100 + e % 4 for e in range(En)]  # the same four seeds under both settings
    rewards, (vs, vp), ext = a.evaluate(seeds=seeds)
    assert rewards.shape[1] == En and vs.shape[1:] == (En, N) and ext["steps"].shape == (En,)
    assert bool((ext["steps"] >= 1).all())
    grouped = group_ext_info(ext, a.group_index)
    assert grouped["count"].tolist() == [4, 4]
    for key in ("steps", "avg_speeds", "crash_rate", "traffic_speeds", "merge_percents"):
        assert grouped[key].shape == (2,) and bool(torch.isfinite(grouped[key]).all()), key
    assert torch.equal(a.env.state, before) and torch.equal(a.obs, b.obs) and torch.equal(a._sample_counter, b._sample_counter)
    ra, rb = a.interact(), b.interact()
    torch.cuda.synchronize()
    for key in KEYS:
        assert torch.equal(ra[key], rb[key]), key
    a.env.poll_errors()
    a.env.close(); b.env.close()
