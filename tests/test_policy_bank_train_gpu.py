"""The policy bank's training half on the MI355X (include/mm_policy_bank_train.h, mm_opt_step_bank of include/mm_opt_step.h,
learner.BankPPOLearner): every member's outputs against mm_policy_eval / mm_policy_train / mm_opt_step on that member alone, bit
for bit; the S+ / S- sums against float64; isolation between members; determinism and graph capture; the learner end to end.

Comparisons are torch.equal on bits unless a bound is stated.  A reference run is computed once per case (lru_cache) and shared."""
import copy
import functools

import numpy as np
import pytest
import torch

import policy_bank_train_util as U
from marl_mass_amd import _cabi as abi
from marl_mass_amd.learner import BankPPOLearner, PPOLearner, _mlp_params
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork, DeviceRollout

pytestmark = pytest.mark.gpu
NAMES = sorted(U.LAYOUTS)


def _lib():
    from marl_mass_amd import hip_library
    return hip_library()


@functools.lru_cache(maxsize=None)
def _members(K, n_s):
    """(actor stacks, critic stacks) of K members: never modified (tests that edit take clones)."""
    return U.stacks(K, n_s, False, 7, "cuda"), U.stacks(K, n_s, True, 7, "cuda")


@functools.lru_cache(maxsize=None)
def _batch(name, with_valid):
    return U.Batch(name, with_valid)


def _scratch(b):
    return torch.empty(_lib().policy_bank_train_scratch_bytes(b.rows, b.row_len, list(b.cols)), dtype=torch.uint8, device="cuda")


def _gathered(b, k):
    idx = b.index(k)
    valid = None if b.valid is None else b.valid[idx].contiguous()
    return idx, b.obs[idx].contiguous(), b.act[idx].contiguous(), b.ret[idx].contiguous(), b.old_logp[idx].contiguous(), valid


# ---- 1. eval
@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_eval_matches_policy_eval_per_member(name, with_valid):
    clib, b = _lib(), _batch(name, with_valid)
    A, Cr = _members(b.K, b.n_s)
    pad, canary = 64, -12345.0
    bufs = [torch.full((b.n + 2 * pad,), canary, device="cuda") for _ in range(2)]
    logp, value = bufs[0][pad:pad + b.n], bufs[1][pad:pad + b.n]
    assert U.bank_eval(clib, b, U.struct(A), U.struct(Cr), logp, value) == abi.MM_OK
    for buf in bufs:  # the outputs sit between canaries that stay intact
        assert bool((buf[:pad] == canary).all()) and bool((buf[pad + b.n:] == canary).all())
    for k in range(b.K):
        idx, obs, act, _, _, valid = _gathered(b, k)
        if idx.numel() == 0:
            continue
        want_lp, want_v = U.pt_eval(clib, obs, act, valid, U.struct(U.member(A, k)), U.struct(U.member(Cr, k)), b.n_s)
        assert torch.equal(logp[idx], want_lp) and torch.equal(value[idx], want_v), (name, k)
        if valid is not None:
            off = valid == 0
            assert bool((logp[idx][off] == 0).all()) and bool((value[idx][off] == 0).all())
    # one network alone
    only = torch.full((b.n,), canary, device="cuda")
    assert U.bank_eval(clib, b, None, U.struct(Cr), None, only) == abi.MM_OK
    assert torch.equal(only, value)
    assert U.bank_eval(clib, b, U.struct(A), None, only, None) == abi.MM_OK
    assert torch.equal(only, logp)


# ---- 2. train
@functools.lru_cache(maxsize=None)
def _bank_run(name, with_valid, form, critic_loss, networks):
    clib, b = _lib(), _batch(name, with_valid)
    A, Cr = _members(b.K, b.n_s)
    with_a, with_c = networks != "critic", networks != "actor"
    ga = [torch.full_like(t, float("nan")) for t in A] if with_a else None
    gc = [torch.full_like(t, float("nan")) for t in Cr] if with_c else None
    mode = "target_value" if form == "reference" else "advantages"
    rc, loss, sums, diag = U.bank_train(clib, b, U.struct(A) if with_a else None, U.struct(Cr) if with_c else None,
                                        U.struct(ga) if with_a else None, U.struct(gc) if with_c else None, form, critic_loss, mode,
                                        _scratch(b))
    assert rc == abi.MM_OK
    torch.cuda.synchronize()
    return loss, sums, diag, ga, gc


def _check_member(b, k, run, form, critic_loss, networks, A, Cr, advantages=None):
    """Member k of a bank run against mm_policy_train on its gathered samples."""
    clib = _lib()
    loss, sums, diag, ga, gc = run
    with_a, with_c = networks != "critic", networks != "actor"
    idx, obs, act, ret, old, valid = _gathered(b, k)
    empty = idx.numel() == 0 or (valid is not None and int(valid.sum()) == 0)
    adv = (b.advantages if advantages is None else advantages)[idx].contiguous()
    want = U.pt_train(clib, obs, act, ret, old, valid, U.struct(U.member(A, k)) if with_a else None,
                      U.struct(U.member(Cr, k)) if with_c else None, b.n_s, critic_loss,
                      sums[k].contiguous() if form == "reference" else None, adv if form == "per_sample" else None)
    assert torch.equal(loss[k], want[0]), (k, loss[k], want[0])
    for mine, theirs in ((ga, want[1]), (gc, want[2])):
        if mine is None:
            continue
        for t, w in zip(mine, theirs):
            assert torch.equal(t[k], w), k
            assert not empty or float(t[k].abs().max()) == 0.0  # exact zeros for an empty or fully masked group
    if empty:
        assert float(loss[k].abs().max()) == 0.0
    for d, w in zip(diag, want[3]):
        if d is not None:
            assert torch.equal(d[idx], w), k


@pytest.mark.parametrize("networks", ["both", "actor", "critic"])
@pytest.mark.parametrize("critic_loss", ["mse", "huber"])
@pytest.mark.parametrize("form", ["reference", "per_sample"])
@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_train_matches_policy_train_per_member(name, with_valid, form, critic_loss, networks):
    """Member k's twelve gradients, two losses and three diagnostics are those of mm_policy_train on the gathered slice: the
    reference form is fed the bank's own adv_sums output, the per-sample form torch's float32 returns - value."""
    b = _batch(name, with_valid)
    A, Cr = _members(b.K, b.n_s)
    run = _bank_run(name, with_valid, form, critic_loss, networks)
    assert bool(torch.isfinite(run[0]).all())
    for k in range(b.K):
        _check_member(b, k, run, form, critic_loss, networks, A, Cr)


@pytest.mark.parametrize("name", ["mixed", "slices"])
def test_target_value_in_the_per_sample_form(name):
    """advantages given directly and as returns - target_value are the same float32 numbers: the same bits."""
    b = _batch(name, True)
    direct = _bank_run(name, True, "per_sample", "mse", "both")
    A, Cr = _members(b.K, b.n_s)
    ga, gc = [torch.full_like(t, float("nan")) for t in A], [torch.full_like(t, float("nan")) for t in Cr]
    rc, loss, _, diag = U.bank_train(_lib(), b, U.struct(A), U.struct(Cr), U.struct(ga), U.struct(gc), "per_sample", "mse",
                                     "target_value", _scratch(b))
    assert rc == abi.MM_OK and torch.equal(loss, direct[0])
    assert all(torch.equal(x, y) for x, y in zip(ga + gc + list(diag), direct[3] + direct[4] + list(direct[2])))


# ---- 3. the adv_sums output
@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_adv_sums_within_one_ulp_of_float64(name, with_valid):
    """S+ sums non-negative terms only and S- non-positive ones: no cancellation, so an fp64 accumulation rounded once lies
    within 1 float32 ulp of the exact sum of the same float32 advantages."""
    b = _batch(name, with_valid)
    sums = _bank_run(name, with_valid, "reference", "mse", "both")[1].cpu().numpy()
    for k in range(b.K):
        idx = b.index(k)
        adv = b.advantages[idx]
        if b.valid is not None:
            adv = adv[b.valid[idx] != 0]
        adv = adv.double().cpu()
        for j, exact in enumerate((float(adv.clamp(min=0).sum()), float(adv.clamp(max=0).sum()))):
            ulp = float(np.spacing(np.float32(abs(exact))))
            print("adv_sums %s k %d %s: %.9g vs %.17g (ulp %.3g)" % (name, k, "+-"[j], sums[k, j], exact, ulp))
            assert abs(float(sums[k, j]) - exact) <= ulp, (name, k, j)


# ---- 4. isolation
def test_members_are_isolated():
    """Perturbing member 1's parameters, samples and mask moves no bit of members 0, 2 and 3 (mixed)."""
    clib, b0 = _lib(), _batch("mixed", True)
    base = _bank_run("mixed", True, "reference", "huber", "both")
    b = copy.copy(b0)
    idx = b0.index(1)
    g = torch.Generator().manual_seed(5)
    b.obs_store, b.act_store, b.ret_store = b0.obs_store.clone(), b0.act_store.clone(), b0.ret_store.clone()
    b.obs, b.act, b.ret = b.obs_store[:, :b.n_s], b.act_store[::3], b.ret_store[::2]
    b.obs[idx] += torch.randn(idx.numel(), b.n_s, generator=g).cuda()
    b.act[idx] = (b.act[idx] + 1) % U.N_A
    b.ret[idx] += 1.0
    b.old_logp, b.target_value, b.valid = b0.old_logp.clone(), b0.target_value.clone(), b0.valid.clone()
    b.old_logp[idx] -= 0.25
    b.target_value[idx] += 0.5
    b.valid[idx] = 1  # (the fully masked group becomes live)
    A, Cr = [[t.clone() for t in net] for net in _members(b.K, b.n_s)]
    for t in A + Cr:
        t[1] += 0.05
    ga, gc = [torch.full_like(t, float("nan")) for t in A], [torch.full_like(t, float("nan")) for t in Cr]
    rc, loss, sums, diag = U.bank_train(clib, b, U.struct(A), U.struct(Cr), U.struct(ga), U.struct(gc), "reference", "huber",
                                        "target_value", _scratch(b))
    assert rc == abi.MM_OK
    assert not torch.equal(loss[1], base[0][1]) and float(ga[0][1].abs().max()) > 0
    for k in (0, 2, 3):
        ik = b0.index(k)
        assert torch.equal(loss[k], base[0][k]) and torch.equal(sums[k], base[1][k])
        assert all(torch.equal(x[k], y[k]) for x, y in zip(ga + gc, base[3] + base[4]))
        assert all(torch.equal(x[ik], y[ik]) for x, y in zip(diag, base[2]))


# ---- 5. determinism and capture
def _synthetic_rollout(T, E, N, S, seed):
    g = torch.Generator().manual_seed(seed)
    return {"states": (torch.randn(T, E, N, S, generator=g) * 1.5).cuda(),
            "actions": torch.randint(0, U.N_A, (T, E, N), generator=g, dtype=torch.int32).cuda(),
            "returns": (torch.randn(T, E, N, generator=g) * 2.0).cuda()}


def _nets(K, n_s, seed):
    torch.manual_seed(seed)
    actors, critics = [ActorNetwork(n_s, 128, U.N_A) for _ in range(K)], [CriticNetwork(n_s, U.N_A, 128, 1) for _ in range(K)]
    with torch.no_grad():
        for a in actors:
            a.fc3.weight.mul_(3.0)
    return [a.cuda() for a in actors], [c.cuda() for c in critics]


def _state_of(learner):
    out = [t for net in learner.params + learner.targets + learner.state1 for t in net] + [learner.steps, learner._grad_norm]
    if learner.state2[0] is not None:
        out += [t for net in learner.state2 for t in net]
    return out


def _member_state(learner, k):
    """Member k's parameters, targets, optimiser state, steps and norms."""
    stacked = [t for net in learner.params + learner.targets + learner.state1 for t in net]
    if learner.state2[0] is not None:
        stacked += [t for net in learner.state2 for t in net]
    return [t[k] for t in stacked] + [learner.steps[:, k], learner._grad_norm[:, k]]


def test_two_calls_give_equal_bits():
    a = _bank_run("big", True, "reference", "mse", "both")
    _bank_run.cache_clear()
    b = _bank_run("big", True, "reference", "mse", "both")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[3] + a[4] + list(a[2]), b[3] + b[4] + list(b[2])))


@pytest.mark.parametrize("optimizer_type", ["rmsprop", "adam"])
def test_train_is_graph_capturable(optimizer_type):
    """A torch.cuda.graph capture of train() -- eval + train + opt step per agent step -- replays to the eager bits."""
    K, groups, T, N, S = 3, [3, 0, 5], 4, 2, 30
    actors, critics = _nets(K, S, 11)
    learner = BankPPOLearner(actors, critics, _lib(), groups, optimizer_type=optimizer_type, target_tau=0.5)
    batch = _synthetic_rollout(T, 8, N, S, 3)
    start = [t.clone() for t in _state_of(learner)]

    def restore():
        for t, s in zip(_state_of(learner), start):
            t.copy_(s)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [l.clone() for l in learner.train(batch, n_episodes=[5, 0, 10])]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    after = [t.clone() for t in _state_of(learner)]
    assert not torch.equal(after[0], start[0])
    restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        glosses = learner.train(batch, n_episodes=[5, 0, 10])
    restore()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(eager, glosses))
    assert all(torch.equal(x, y) for x, y in zip(after, _state_of(learner)))


# ---- 6. mm_opt_step_bank
def _opt_group(algo, tensors, grads, s1, s2, targets, step, norm, clip, soft):
    g = abi.MMOptGroup()
    g.algo, g.n_tensors = algo, len(tensors)
    for i, t in enumerate(tensors):
        g.count[i] = t.numel()
        g.param[i], g.grad[i], g.state1[i], g.target[i] = t.data_ptr(), grads[i].data_ptr(), s1[i].data_ptr(), targets[i].data_ptr()
        if s2 is not None:
            g.state2[i] = s2[i].data_ptr()
    g.step, g.grad_norm = step.data_ptr(), norm.data_ptr()
    g.lr, g.eps, g.max_grad_norm, g.tau, g.soft_update = 1e-3, 1e-8, (0.5 if clip else -1.0), 0.25, int(soft)
    g.alpha_or_beta1, g.beta2 = (0.9, 0.999) if algo == abi.OPT_ADAM else (0.99, 0.0)
    return g


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("K", [1, 3, 64])
@pytest.mark.parametrize("algo", ["rmsprop", "adam"])
def test_opt_step_bank_matches_opt_step_per_member(algo, K, clip):
    """Two prototype groups (the real actor and critic shapes at n_s = 25: odd tensor sizes) x K members against K calls of
    mm_opt_step on the members' own tensors; Adam with a different step counter per member; some soft_mask bits set."""
    clib, code = _lib(), abi.OPT_ADAM if algo == "adam" else abi.OPT_RMSPROP
    soft_mask = 0b1011 | (1 << 40) | (1 << 63)
    g = torch.Generator().manual_seed(K)
    nets = []
    for critic in (False, True):
        P = U.stacks(K, 25, critic, 3, "cuda")
        new = lambda scale, pos=False: [((torch.rand(t.shape, generator=g) if pos else torch.randn(t.shape, generator=g)) * scale).cuda() for t in P]  # noqa: E731
        nets.append({"p": P, "g": new(0.05), "s1": new(1e-3, True), "s2": new(1e-3, True) if algo == "adam" else None,
                     "t": new(0.3), "step": (torch.arange(K, dtype=torch.int32) * 3 + (1 if critic else 0)).cuda(),
                     "norm": torch.full((K,), float("nan")).cuda()})
    want = []
    for k in range(K):  # the reference: mm_opt_step on clones of member k's tensors
        clones, groups = [], []
        for net in nets:
            c = {key: ([t[k].clone() for t in net[key]] if isinstance(net[key], list) else None) for key in ("p", "g", "s1", "s2", "t")}
            c["step"], c["norm"] = net["step"][k:k + 1].clone(), net["norm"][k:k + 1].clone()
            clones.append(c)
            groups.append(_opt_group(code, c["p"], c["g"], c["s1"], c["s2"], c["t"], c["step"], c["norm"], clip, (soft_mask >> k) & 1))
        clib.opt_step(groups, U._stream())
        want.append(clones)
    protos = [_opt_group(code, net["p"], net["g"], net["s1"], net["s2"], net["t"], net["step"], net["norm"], clip, 0) for net in nets]
    for proto, net in zip(protos, nets):
        for i in range(6):
            proto.count[i] = net["p"][i][0].numel()
    kept = [[t.clone() for t in net["g"]] for net in nets]
    clib.opt_step_bank(protos, K, soft_mask, U._stream())
    torch.cuda.synchronize()
    for k in range(K):
        for net, ref, g0 in zip(nets, want[k], kept):
            for key in ("p", "s1", "s2", "t"):
                if net[key] is not None:
                    assert all(torch.equal(t[k], w) for t, w in zip(net[key], ref[key])), (k, key)
            assert all(torch.equal(t, w) for t, w in zip(net["g"], g0))  # the gradients are read only
            assert int(net["step"][k]) == int(ref["step"][0]) and torch.equal(net["norm"][k:k + 1], ref["norm"])
    moved = [bool((soft_mask >> k) & 1) for k in range(K)]
    assert any(moved) and (K == 1 or not all(moved))


# ---- 7. the learner
def test_learner_end_to_end():
    """v1, E = 8, N = 4, DeviceRollout in bank mode with group_envs [3, 0, 5], T = 5, two train() calls with n_episodes
    [5, 0, 10]: every member against a K = 1 learner on its slice (bits), and the first agent step against PPOLearner."""
    from marl_mass_amd import VecMergeEnv
    E, N, T, groups, eps = 8, 4, 5, [3, 0, 5], [5, 0, 10]
    clib = _lib()
    actors, critics = _nets(3, 30, 21)
    first = [(copy.deepcopy(a), copy.deepcopy(c)) for a, c in zip(actors, critics)]
    env = VecMergeEnv(E, N, seed=9, config={"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}, cbf_eta=0.03125, qp_solver="exact",
                      cbf_tau=0.5, auto_reset=True)
    ro = DeviceRollout(env, actors, critics, roll_out_n_steps=T, sample_seed=4, group_envs=groups)
    assert ro.bank_mode and ro.fused_policy
    kw = dict(target_tau=0.5, optimizer_type="adam")
    bank = BankPPOLearner(actors, critics, clib, groups, **kw)
    for net, members in enumerate((actors, critics)):  # the modules' parameters and gradients alias the stacks
        for k, m in enumerate(members):
            for i, p in enumerate(_mlp_params(m)):
                assert p.data_ptr() == bank.params[net][i][k].data_ptr() and p.grad.data_ptr() == bank.grads[net][i][k].data_ptr()
    solo = [BankPPOLearner([copy.deepcopy(a)], [copy.deepcopy(c)], clib, [groups[k]], **kw) for k, (a, c) in enumerate(first)]
    ppo = [PPOLearner(copy.deepcopy(a), copy.deepcopy(c), clib, fused_step=True, **kw) for a, c in first]
    for rnd in range(2):
        out = ro.interact()
        if rnd == 1:  # the rollout acted with the updated weights: its stack is the learner's
            assert all(torch.equal(t, s) for t, s in zip(ro.bank.tensors, bank.params[0]))
            assert not torch.equal(ro.bank.W1[0], first[0][0].fc1.weight.detach())
        losses = bank.train(out, n_episodes=eps)
        assert len(losses) == N and all(tuple(l.shape) == (3, 2) for l in losses)
        for k in range(3):
            sl = ro.group_slice(k)
            part = {key: out[key][:, sl] for key in ("states", "actions", "returns")}
            solo_losses = solo[k].train(part, n_episodes=eps[k])
            assert all(torch.equal(l[k], s[0]) for l, s in zip(losses, solo_losses)), k
            assert all(torch.equal(x, y) for x, y in zip(_member_state(bank, k), _member_state(solo[k], 0))), k
            if rnd == 0 and groups[k] > 0:  # the first agent step against PPOLearner(fused_step=True) on the slice
                want = ppo[k].train(part, n_episodes=eps[k])[0]
                got = losses[0][k]
                assert torch.equal(got[1], want[1]), (k, got, want)  # the critic loss: the same kernel arithmetic
                st = part["states"].reshape(-1, N, 30)[:, 0, :].float()
                ac, rt = part["actions"].reshape(-1, N)[:, 0].int(), part["returns"].reshape(-1, N)[:, 0].float()
                ref = PPOLearner(copy.deepcopy(first[k][0]), copy.deepcopy(first[k][1]), clib)
                adv = ref.advantages(st, ac, rt)
                n_k = adv.numel()
                bound = 2.0 * n_k * 2.0 ** -24 * float(adv.abs().double().sum()) / n_k
                print("member %d actor loss %.9g vs PPOLearner %.9g (bound %.3g)" % (k, float(got[0]), float(want[0]), bound))
                assert abs(float(got[0]) - float(want[0])) <= bound, (k, float(got[0]), float(want[0]), bound)
    assert bank.steps.tolist() == [[2 * N] * 3, [2 * N] * 3]
    assert tuple(bank.last_grad_norm().shape) == (3, 2)
    # members 0 and 2 blended their targets (n_episodes 5 and 10), member 1 (0 episodes) did not
    assert torch.equal(bank.targets[0][0][1], first[1][0].fc1.weight.detach())
    assert not torch.equal(bank.targets[0][0][0], first[0][0].fc1.weight.detach())
    # a member's optimiser state moves to a PPOLearner and back
    sd = bank.optimizer_state_dict(0)
    ppo[1].load_optimizer_state_dict(sd)
    back = ppo[1].optimizer_state_dict()
    bank.load_optimizer_state_dict(2, back)
    assert int(bank.steps[0, 2]) == int(bank.steps[0, 0]) == 2 * N
    for net in range(2):
        assert all(torch.equal(t[2], t[0]) for t in bank.state1[net] + bank.state2[net])


def test_learner_refuses_a_batch_that_does_not_match_group_envs():
    actors, critics = _nets(2, 30, 2)
    learner = BankPPOLearner(actors, critics, _lib(), [3, 5])
    with pytest.raises(ValueError, match="do not match the batch"):
        learner.train(_synthetic_rollout(2, 7, 2, 30, 1))
    with pytest.raises(ValueError, match="do not match the batch"):
        learner.evaluate(torch.zeros(16, 30, device="cuda"), torch.zeros(16, dtype=torch.int32, device="cuda"), 2, col_start=[0, 3, 9])
    with pytest.raises(ValueError, match="one int per member"):
        learner.train(_synthetic_rollout(2, 8, 2, 30, 1), n_episodes=[5, 5, 5])
    with pytest.raises(ValueError, match="one non-negative env count per member"):
        BankPPOLearner(*_nets(2, 30, 2), _lib(), [8])
