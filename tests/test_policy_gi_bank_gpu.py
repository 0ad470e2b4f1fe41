"""mm_policy_gi_bank_act (include/mm_policy_gi_bank.h) and DeviceRollout's bank mode with shared members on the MI355X.

The existing single-network entry is the reference: group k's log-probability rows and values are bit-equal to mm_policy_gi_act
on that slice with member k's weights, the actions are mm_sample_actions' draws from the bank's own rows at the global agent
index, and rows and values agree with the float64 module under policy_act_util.compare (the rule and the factor of the
mm_policy_gi_act tests).  Members and the float64 reference: policy_gi_bank_util; layouts: policy_bank_util."""
import copy

import numpy as np
import pytest
import torch

import policy_act_util as U
import policy_gi_bank_util as G
from marl_mass_amd import VecMergeEnv, _cabi as abi, hip_library
from marl_mass_amd.rollout import DeviceRollout, group_ext_info

pytestmark = pytest.mark.gpu

DEV = "cuda"
ERRORS = {}
V1 = dict(config={"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}, cbf_eta=0.03125, qp_solver="exact", cbf_tau=0.5, seed=9,
          auto_reset=True)
KEYS = ("states", "actions", "returns", "dones", "average_speed", "min_headway")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _members(n_s, K):
    return [copy.deepcopy(G.member(n_s, k)).to(DEV) for k in range(K)]


def _single(clib, net, obs, seed, ctr):
    """mm_policy_gi_act on obs with one member: {actions, logp, value, counter}."""
    return U.run(clib, "gi", U.weights_of("gi", net), obs.contiguous(), G.N_A, seed, ctr)


def _bank(clib, params, obs, K, start, ctr=G.CTR, actions=True, logp=True, value=True, counter=True, guarded=False):
    """One well-formed bank launch into fresh sentinel-filled outputs: {actions, logp, value, counter (tensor), check}."""
    n, n_s = obs.shape
    checks = []

    def buf(elems, dtype, fill, on):
        if not on:
            return None
        if guarded:
            v, chk = U.guarded(elems, dtype, DEV)
            checks.append(chk)
            return v
        return torch.full((elems,), fill, dtype=dtype, device=DEV)

    out = {"actions": buf(n, torch.int32, -1, actions), "logp": buf(n * G.N_A, torch.float32, float("nan"), logp),
           "value": buf(n, torch.float32, float("nan"), value), "counter": U.counter_tensor(ctr, DEV) if counter else None}
    assert G.launch_bank(clib, params, obs, n, n_s, K, G.c_groups(start), G.SEED, out["counter"], out["actions"], out["logp"],
                         out["value"]) == abi.MM_OK
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    if logp:
        out["logp"] = out["logp"].view(n, G.N_A)
    return out


@pytest.mark.parametrize("n_s", G.NS)
@pytest.mark.parametrize("name", sorted(G.LAYOUTS))
def test_layout(name, n_s):
    clib = hip_library()
    sizes = G.LAYOUTS[name]
    K, n, start = len(sizes), int(sum(sizes)), G.group_start(sizes)
    members = _members(n_s, K)
    tensors = G.stack(members, DEV)
    params = G.bank_params(tensors)
    obs = G.obs_of(n_s, n).to(DEV)
    # ---- guarded buffers at an offset of one element, all three outputs
    out = _bank(clib, params, obs, K, start, guarded=True)
    actions, logp, value = out["actions"], out["logp"], out["value"]
    assert U.counter_value(out["counter"]) == G.CTR + 1
    assert bool(torch.isfinite(logp).all()) and bool(torch.isfinite(value).all())
    assert bool(((actions >= 0) & (actions < G.N_A)).all())
    # ---- 4. output modes
    o = _bank(clib, params, obs, K, start, logp=False, value=False, guarded=True)  # logp = NULL: the same actions
    assert torch.equal(o["actions"], actions) and U.counter_value(o["counter"]) == G.CTR + 1
    o = _bank(clib, params, obs, K, start, actions=False, counter=False, guarded=True)  # nothing sampled, no counter needed
    assert torch.equal(_bits(o["logp"]), _bits(logp)) and torch.equal(_bits(o["value"]), _bits(value))
    o = _bank(clib, params, obs, K, start, actions=False, guarded=True)  # ... and a counter that is given is left alone
    assert torch.equal(_bits(o["logp"]), _bits(logp)) and U.counter_value(o["counter"]) == G.CTR
    o = _bank(clib, params, obs, K, start, actions=False, logp=False, counter=False, guarded=True)  # value only
    assert torch.equal(_bits(o["value"]), _bits(value))
    # ---- 1. rows of group k == mm_policy_gi_act on the slice with member k, bit for bit
    f32 = {"logp": torch.empty(n, G.N_A, device=DEV), "value": torch.empty(n, device=DEV)}
    for k in range(K):
        lo, hi = start[k], start[k + 1]
        if hi == lo:
            continue
        one = _single(clib, members[k], obs[lo:hi], G.SEED, G.CTR)
        assert torch.equal(_bits(logp[lo:hi]), _bits(one["logp"])), (name, k)
        assert torch.equal(_bits(value[lo:hi]), _bits(one["value"])), (name, k)
        if K == 1:
            assert torch.equal(actions, one["actions"]), name
        elif not torch.equal(tensors[6][k], tensors[6][(k + 1) % K]):
            wrong = _single(clib, members[(k + 1) % K], obs[lo:hi], G.SEED, G.CTR)
            assert not torch.equal(_bits(logp[lo:hi]), _bits(wrong["logp"])), (name, k)  # a wrong member cannot pass
            assert not torch.equal(_bits(value[lo:hi]), _bits(wrong["value"])), (name, k)
        with torch.no_grad():
            f32["logp"][lo:hi] = members[k](obs[lo:hi])
            f32["value"][lo:hi] = members[k](obs[lo:hi], out_type="v")[:, 0]
    # ---- 2. actions == mm_sample_actions on the bank's own rows, global index; and the float64 inverse CDF outside BAND
    own, c = U.sample(clib, logp, G.SEED, G.CTR)
    assert torch.equal(actions, own) and c == G.CTR + 1
    near = G.near(n_s, sizes)
    assert near.mean() <= U.BAND_SHARE
    assert np.array_equal(actions.cpu().numpy()[~near], G.actions64(n_s, sizes)[~near]), name
    # ---- 3. the float64 module forward, under the mm_policy_gi_act tests' rule and factor
    U.compare(ERRORS, "%s_s%d" % (name, n_s), {"logp": logp, "value": value}, f32,
              {"logp": G.logp64_of(n_s, sizes), "value": G.value64_of(n_s, sizes)})
    assert float(torch.logsumexp(logp.double(), -1).abs().max()) <= 1e-6


def test_results_do_not_depend_on_the_split():
    """The same 65 548 rows under one member as K = 1, as (65 541, 7) and as 64 uneven groups of identical members: one set of
    bits, mm_policy_gi_act's (tile origin, workgroup count and persistent stride all differ between the three launches)."""
    clib = hip_library()
    n, n_s = 65548, 30
    obs = G.obs_of(n_s, n).to(DEV)
    net = copy.deepcopy(G.member(n_s, 0)).to(DEV)
    want = _single(clib, net, obs, G.SEED, G.CTR)
    sizes64 = [1 + 30 * k for k in range(63)]
    sizes64.append(n - sum(sizes64))
    for sizes in ((n,), (65541, 7), tuple(sizes64)):
        K = len(sizes)
        out = _bank(clib, G.bank_params(G.stack([net] * K, DEV)), obs, K, G.group_start(sizes))
        assert torch.equal(out["actions"], want["actions"]), K
        assert torch.equal(_bits(out["logp"]), _bits(want["logp"])) and torch.equal(_bits(out["value"]), _bits(want["value"])), K


def test_refusals():
    """Every refused call returns MM_ERR_INVALID_ARG with the outputs at their fill and the counter unchanged; n = 0 is MM_OK
    and leaves the counter alone too."""
    clib = hip_library()
    n_s = 30
    K, n, start = 3, 65, G.group_start((1, 31, 33))
    tensors = G.stack(_members(n_s, K), DEV)
    obs = G.obs_of(n_s, n).to(DEV)
    actions = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    logp = torch.full((n, G.N_A), float("nan"), device=DEV)
    value = torch.full((n,), float("nan"), device=DEV)
    ctr = U.counter_tensor(G.CTR, DEV)
    ok = dict(params=G.bank_params(tensors), obs=obs, n=n, n_s=n_s, K=K, start=G.c_groups(start), seed=G.SEED, counter=ctr,
              actions=actions, logp=logp, value=value, hidden=128, n_a=G.N_A)
    refused = [("obs NULL", dict(obs=None)), ("bank NULL", dict(params=None)), ("group_start NULL", dict(start=None)),
               ("actions without counter", dict(counter=None)), ("no output", dict(actions=None, logp=None, value=None)),
               ("no output, no counter", dict(actions=None, logp=None, value=None, counter=None)),
               ("K 0", dict(K=0)), ("K 65", dict(K=65, start=G.c_groups([0] * 65 + [n]))),
               ("hidden 512", dict(hidden=512)), ("hidden 64", dict(hidden=64)), ("n_s 24", dict(n_s=24)), ("n_s 33", dict(n_s=33)),
               ("n_a 0", dict(n_a=0)), ("n_a 9", dict(n_a=9)), ("n < 0", dict(n=-1, start=G.c_groups([0, 0, 0, -1]))),
               ("group_start[0] != 0", dict(start=G.c_groups([1, 1, 32, 65]))),
               ("group_start decreases", dict(start=G.c_groups([0, 40, 32, 65]))),
               ("group_start ends short of n", dict(start=G.c_groups([0, 1, 32, 64]))),
               ("group_start ends past n", dict(start=G.c_groups([0, 1, 32, 66])))]
    refused += [("member base %s NULL" % abi.GI_PARAMS[j], dict(params=G.bank_params(tensors, null=j))) for j in range(12)]
    for what, change in refused:
        assert G.launch_bank(clib, **dict(ok, **change)) == abi.MM_ERR_INVALID_ARG, what
    assert G.launch_bank(clib, **dict(ok, n=0, start=G.c_groups([0, 0, 0, 0]))) == abi.MM_OK
    torch.cuda.synchronize()
    assert bool((actions == -7).all()) and bool(torch.isnan(logp).all()) and bool(torch.isnan(value).all())
    assert U.counter_value(ctr) == G.CTR
    assert G.launch_bank(clib, **ok) == abi.MM_OK  # and the well-formed call goes through
    torch.cuda.synchronize()
    assert bool((actions >= 0).all()) and bool(torch.isfinite(logp).all()) and bool(torch.isfinite(value).all())
    assert U.counter_value(ctr) == G.CTR + 1


def test_graph_capture_replays_draw_fresh_numbers():
    """Two bank launches captured into one single-chain graph, replayed twice: each replay equals the eager sequence at the
    same counter values; the host group table is overwritten after the capture (the launch carries its own copy)."""
    clib = hip_library()
    n_s, sizes = 30, (1, 31, 33)
    K, n, start = 3, 65, G.group_start(sizes)
    params = G.bank_params(G.stack(_members(n_s, K), DEV))
    obs = G.obs_of(n_s, n).to(DEV)

    def eager(c0):
        ctr, outs = U.counter_tensor(c0, DEV), []
        for _ in range(4):
            a = torch.full((n,), -1, dtype=torch.int32, device=DEV)
            v = torch.full((n,), float("nan"), device=DEV)
            assert G.launch_bank(clib, params, obs, n, n_s, K, G.c_groups(start), G.SEED, ctr, a, None, v) == abi.MM_OK
            outs.append((a, v))
        torch.cuda.synchronize()
        assert U.counter_value(ctr) == c0 + 4
        return outs

    want = eager(G.CTR)
    assert not torch.equal(want[0][0], want[1][0])
    ctr = U.counter_tensor(G.CTR, DEV)
    a1, a2 = (torch.full((n,), -1, dtype=torch.int32, device=DEV) for _ in range(2))
    v1, v2 = (torch.full((n,), float("nan"), device=DEV) for _ in range(2))
    table = G.c_groups(start)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        assert G.launch_bank(clib, params, obs, n, n_s, K, table, G.SEED, ctr, a1, None, v1) == abi.MM_OK
        assert G.launch_bank(clib, params, obs, n, n_s, K, table, G.SEED, ctr, a2, None, v2) == abi.MM_OK
    for k in range(K + 1):
        table[k] = 0
    assert U.counter_value(ctr) == G.CTR  # a capture runs nothing
    for r in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a1, want[2 * r][0]) and torch.equal(a2, want[2 * r + 1][0]), r
        assert torch.equal(_bits(v1), _bits(want[2 * r][1])) and torch.equal(_bits(v2), _bits(want[2 * r + 1][1])), r
        assert U.counter_value(ctr) == G.CTR + 2 * (r + 1)


# ---- DeviceRollout's bank mode with shared members: v1 MASS, exact QP, E = 16, N = 4, T = 4, K = 4
E, N, T, K4 = 16, 4, 4, 4


def _bank_rollout(nets, **kw):
    return DeviceRollout(VecMergeEnv(E, N, **V1), nets, roll_out_n_steps=T, sample_seed=4, group_envs=[4] * K4, **kw)


def test_rollout_identical_members_equal_single_network_twin():
    """Four identical members: every tensor of interact() -- `returns` included, the bootstrap value being the same arithmetic --
    is bit-equal to a single-network shared DeviceRollout twin with the same seeds."""
    net = copy.deepcopy(G.member(30, 0)).to(DEV)
    twin = DeviceRollout(VecMergeEnv(E, N, **V1), net, roll_out_n_steps=T, sample_seed=4)
    bank = _bank_rollout([copy.deepcopy(net) for _ in range(K4)])
    assert bank.fused_policy and twin.fused_policy and bank.shared and bank.bank is None and bank.shared_bank.K == K4
    assert bank.group_index.tolist() == [k for k in range(K4) for _ in range(4)] and bank.group_slice(2) == slice(8, 12)
    for it in range(2):
        a, b = twin.interact(), bank.interact()
        torch.cuda.synchronize()
        for key in KEYS:
            assert torch.equal(a[key], b[key]), (it, key)
        assert torch.equal(twin.env.state.cpu(), bank.env.state.cpu()) and int(twin._sample_counter) == int(bank._sample_counter)
    assert int(bank._sample_counter) == 2 * (T + 1)
    twin.env.poll_errors(); bank.env.poll_errors()
    twin.env.close(); bank.env.close()


def test_rollout_distinct_members_act_on_their_own_groups():
    """Four members (three distinct): actions[t] is reproduced from states[t] by per-slice mm_policy_gi_act rows plus ONE
    mm_sample_actions at counter value t; the bootstrap draws once more."""
    clib = hip_library()
    nets = _members(30, K4)
    ro = _bank_rollout(nets)
    assert ro.fused_policy and ro.shared_bank is not None
    out = ro.interact()
    torch.cuda.synchronize()
    differs = 0
    for t in range(T):
        flat = out["states"][t].reshape(E * N, 30)
        rows = torch.cat([_single(clib, nets[k], flat[16 * k:16 * k + 16], 4, t)["logp"] for k in range(K4)])
        want, _ = U.sample(clib, rows, 4, t)
        assert torch.equal(out["actions"][t].view(-1), want), t
        alone = _single(clib, nets[0], flat, 4, t)["actions"]
        differs += int((alone != want).sum())
    assert differs > 0  # member 0 alone would have acted differently
    assert int(ro._sample_counter) == T + 1  # the bootstrap's draw
    # the fallback (fused_policy off: members' forwards + one mm_sample_actions) is the same stream up to float32 rows
    fb = _bank_rollout(nets, fused_policy=False)
    assert not fb.fused_policy and fb.shared_bank is None
    assert torch.equal(fb.interact()["states"][0], out["states"][0]) and int(fb._sample_counter) == T + 1
    ro.env.close(); fb.env.close()


def test_rollout_graph_sees_an_edited_member():
    """use_graph=True with an in-place edit of one member between two replays: the bits of an eager twin given the same edit
    (interact() refreshes the stack the captured launches read)."""
    en, gn = _members(30, K4), _members(30, K4)
    eager, graph = _bank_rollout(en), _bank_rollout(gn, use_graph=True)
    assert graph.fused_policy
    graph.interact()  # warm-up + capture + first replay = 2 rollouts
    eager.interact(); eager.interact()
    for it in range(3):
        if it == 1:
            with torch.no_grad():
                for nets in (en, gn):
                    nets[2].actor_linear.weight.mul_(-3.0)
                    nets[2].fc11.bias.add_(0.5)
                    nets[2].critic_linear.bias.add_(1.5)
        a, b = eager.interact(), graph.interact()
        torch.cuda.synchronize()
        for key in KEYS:
            assert torch.equal(a[key], b[key]), (it, key)
        assert torch.equal(eager.env.state.cpu(), graph.env.state.cpu()), it
    # the edit reached the graph's launches: the edited member's stack rows are the new weights
    assert torch.equal(graph.shared_bank.Wa[2], gn[2].actor_linear.weight.detach())
    assert torch.equal(graph.shared_bank.bc[2], gn[2].critic_linear.bias.detach())
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
    assert a.fused_policy and a.shared_bank is not None
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
