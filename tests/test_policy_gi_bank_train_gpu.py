"""The shared actor-critic bank's training half on the MI355X (include/mm_policy_gi_bank_train.h, learner.SharedBankPPOLearner):
every member's outputs against mm_policy_gi_act / mm_policy_gi_train / SharedPPOLearner on that member alone, bit for bit; the
S+ / S- sums against float64; isolation between members; determinism and graph capture; refused calls; the learner end to end.

Comparisons are torch.equal on bits unless a bound is stated.  A bank run is computed once per case (lru_cache) and shared."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import policy_gi_bank_train_util as U
from marl_mass_amd import _cabi as abi
from marl_mass_amd.learner import SharedBankPPOLearner, SharedPPOLearner, _params
from marl_mass_amd.rollout import ActorCriticNetwork, DeviceRollout

pytestmark = pytest.mark.gpu
NAMES = sorted(U.LAYOUTS)


def _lib():
    from marl_mass_amd import hip_library
    return hip_library()


@functools.lru_cache(maxsize=None)
def _members(K):
    """The twelve stacks of K members: never modified (tests that edit take clones)."""
    return U.stacks(K, 7, "cuda")


@functools.lru_cache(maxsize=None)
def _batch(name, with_valid):
    return U.Batch(name, with_valid)


def _scratch(b, cols=None):
    need = _lib().policy_gi_bank_train_scratch_bytes(b.rows, b.row_len, list(b.cols if cols is None else cols))
    return torch.empty(need, dtype=torch.uint8, device="cuda")


def _gathered(b, k):
    idx = b.index(k)
    valid = None if b.valid is None else b.valid[idx].contiguous()
    return idx, b.obs[idx].contiguous(), b.act[idx].contiguous(), b.ret[idx].contiguous(), b.old_logp[idx].contiguous(), valid


# ---- 1. eval
@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_eval_matches_policy_gi_act_per_member(name, with_valid):
    clib, b = _lib(), _batch(name, with_valid)
    W = _members(b.K)
    pad, canary = 64, -12345.0
    bufs = [torch.full((b.n + 2 * pad,), canary, device="cuda") for _ in range(2)]
    logp, value = bufs[0][pad:pad + b.n], bufs[1][pad:pad + b.n]
    assert U.bank_eval(clib, b, U.struct(W), logp, value) == abi.MM_OK
    for buf in bufs:  # the outputs sit between canaries that stay intact
        assert bool((buf[:pad] == canary).all()) and bool((buf[pad + b.n:] == canary).all())
    for k in range(b.K):
        idx, obs, act, _, _, valid = _gathered(b, k)
        if idx.numel() == 0:
            continue
        rows, want_v = U.gi_act(clib, obs, U.member(W, k), b.n_s)
        want_lp = rows.gather(1, act.long().clamp(0, U.N_A - 1).unsqueeze(1)).squeeze(1)
        if valid is not None:
            off = valid == 0
            want_lp, want_v = want_lp.masked_fill(off, 0.0), want_v.masked_fill(off, 0.0)
            assert bool((logp[idx][off] == 0).all()) and bool((value[idx][off] == 0).all())
        assert torch.equal(logp[idx], want_lp) and torch.equal(value[idx], want_v), (name, k)
    # either output alone
    only = torch.full((b.n,), canary, device="cuda")
    assert U.bank_eval(clib, b, U.struct(W), None, only) == abi.MM_OK
    assert torch.equal(only, value)
    assert U.bank_eval(clib, b, U.struct(W), only, None) == abi.MM_OK
    assert torch.equal(only, logp)


def test_eval_clamps_actions_out_of_range():
    clib, b0 = _lib(), _batch("mixed", False)
    b = copy.copy(b0)
    b.act_store = b0.act_store.clone()
    b.act = b.act_store[::3]
    b.act[::2] = 99
    b.act[1::2] = -7
    W = _members(b.K)
    logp = torch.full((b.n,), float("nan"), device="cuda")
    assert U.bank_eval(clib, b, U.struct(W), logp, None) == abi.MM_OK
    for k in range(b.K):
        idx = b.index(k)
        if idx.numel():
            rows, _ = U.gi_act(clib, b.obs[idx].contiguous(), U.member(W, k), b.n_s)
            want = rows.gather(1, b.act[idx].long().clamp(0, U.N_A - 1).unsqueeze(1)).squeeze(1)
            assert torch.equal(logp[idx], want), k


# ---- 2. train
@functools.lru_cache(maxsize=None)
def _bank_run(name, with_valid, form, critic_loss):
    clib, b = _lib(), _batch(name, with_valid)
    W = _members(b.K)
    G = [torch.full_like(t, float("nan")) for t in W]
    rc, loss, sums, diag = U.bank_train(clib, b, U.struct(W), U.struct(G), form, critic_loss, _scratch(b))
    assert rc == abi.MM_OK
    torch.cuda.synchronize()
    return loss, sums, diag, G


def _check_member(b, k, run, form, critic_loss, W):
    """Member k of a bank run against mm_policy_gi_train on its gathered samples."""
    clib = _lib()
    loss, sums, diag, G = run
    idx, obs, act, ret, old, valid = _gathered(b, k)
    empty = idx.numel() == 0 or (valid is not None and int(valid.sum()) == 0)
    want = U.gi_train(clib, obs, act, ret, old, valid, U.member(W, k), b.n_s, critic_loss,
                      sums[k].contiguous() if form == "reference" else None)
    assert torch.equal(loss[k], want[0]), (k, loss[k], want[0])
    for t, w in zip(G, want[1]):
        assert torch.equal(t[k], w), k
        assert not empty or float(t[k].abs().max()) == 0.0  # exact zeros for an empty or fully masked group
    if empty:
        assert float(loss[k].abs().max()) == 0.0
    for d, w in zip(diag, want[2]):
        assert torch.equal(d[idx], w), k


@pytest.mark.parametrize("critic_loss", ["mse", "huber"])
@pytest.mark.parametrize("form", ["reference", "per_sample"])
@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_train_matches_policy_gi_train_per_member(name, with_valid, form, critic_loss):
    """Member k's twelve gradients, three losses and three diagnostics are those of mm_policy_gi_train on the gathered slice; the
    reference form is fed the bank's own adv_sums output."""
    b = _batch(name, with_valid)
    W = _members(b.K)
    run = _bank_run(name, with_valid, form, critic_loss)
    assert bool(torch.isfinite(run[0]).all()) and all(bool(torch.isfinite(g).all()) for g in run[3])
    if form == "per_sample":
        assert float(run[1].abs().max()) == 0.0  # no sums in the per-sample form
    for k in range(b.K):
        _check_member(b, k, run, form, critic_loss, W)


# ---- 3. the adv_sums output
@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_adv_sums_within_one_ulp_of_float64(name, with_valid):
    """S+ sums non-negative terms only and S- non-positive ones: no cancellation, so an fp64 accumulation rounded once lies
    within 1 float32 ulp of the exact sum of the same float32 advantages returns - value_now."""
    b = _batch(name, with_valid)
    sums = _bank_run(name, with_valid, "reference", "mse")[1].cpu().numpy()
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
def _same_member(run, base, b, k, k0=None):
    k0 = k if k0 is None else k0
    return (torch.equal(run[0][k], base[0][k0]) and torch.equal(run[1][k], base[1][k0])
            and all(torch.equal(x[k], y[k0]) for x, y in zip(run[3], base[3])))


def test_members_are_isolated_from_other_members_parameters_and_samples():
    """Members 1 and 3 of `mixed` get other parameters, NaN observations and returns and actions out of range; no bit of
    members 0 and 2 moves (member 0 is the empty group)."""
    clib, b0 = _lib(), _batch("mixed", True)
    base = _bank_run("mixed", True, "reference", "huber")
    b = copy.copy(b0)
    b.obs_store, b.act_store, b.ret_store = b0.obs_store.clone(), b0.act_store.clone(), b0.ret_store.clone()
    b.obs, b.act, b.ret = b.obs_store[:, :b.n_s], b.act_store[::3], b.ret_store[::2]
    b.old_logp, b.target_value, b.valid = b0.old_logp.clone(), b0.target_value.clone(), b0.valid.clone()
    W = [t.clone() for t in _members(b.K)]
    for k in (1, 3):
        idx = b0.index(k)
        b.obs[idx] = float("nan")
        b.ret[idx] = float("nan")
        b.act[idx] = 1000 + k
        b.valid[idx] = 1  # (the fully masked group becomes live)
        for t in W:
            t[k] += 0.05
    G = [torch.full_like(t, float("nan")) for t in W]
    rc, loss, sums, diag = U.bank_train(clib, b, U.struct(W), U.struct(G), "reference", "huber", _scratch(b))
    assert rc == abi.MM_OK
    run = (loss, sums, diag, G)
    assert bool(torch.isnan(loss[3]).any())  # the poison reached its own member
    for k in (0, 2):
        ik = b0.index(k)
        assert _same_member(run, base, b, k), k
        assert all(torch.equal(x[ik], y[ik]) for x, y in zip(diag, base[2]))


def test_members_are_isolated_from_other_groups_widths():
    """`mixed` with the groups around member 2 (one column) resized: (0, 0, 5, 6, 23) -> (0, 3, 5, 6, 23), and -> (0, 0, 1, 2, 23)
    on a batch whose columns 1 and 5 are swapped, so that member 2's column sits elsewhere.  Member 2's samples are the same, so
    are its bits."""
    clib, b0 = _lib(), _batch("mixed", True)
    base = _bank_run("mixed", True, "per_sample", "mse")
    W = _members(b0.K)
    for cols in ((0, 3, 5, 6, 23), (0, 0, 1, 2, 23)):
        b = copy.copy(b0)
        b.cols = cols
        if cols[2] != b0.cols[2]:  # move member 2's column (index 5) to column 1: swap the two columns of every array
            perm = torch.arange(b0.n, device="cuda").view(b0.rows, b0.row_len).clone()
            perm[:, [1, 5]] = perm[:, [5, 1]]
            perm = perm.reshape(-1)
            b.obs, b.act, b.ret = b0.obs[perm].contiguous(), b0.act[perm].contiguous(), b0.ret[perm].contiguous()
            b.old_logp, b.target_value, b.valid = b0.old_logp[perm].contiguous(), b0.target_value[perm].contiguous(), b0.valid[perm].contiguous()
        G = [torch.full_like(t, float("nan")) for t in W]
        rc, loss, sums, diag = U.bank_train(clib, b, U.struct(W), U.struct(G), "per_sample", "mse", _scratch(b, cols))
        assert rc == abi.MM_OK
        assert _same_member((loss, sums, diag, G), base, b, 2), cols
        i0, i1 = b0.index(2), U.gather_index(b.rows, b.row_len, cols, 2, "cuda")
        assert all(torch.equal(x[i1], y[i0]) for x, y in zip(diag, base[2]))


# ---- 5. determinism and capture
def test_two_calls_give_equal_bits():
    a = _bank_run("big", True, "reference", "mse")
    _bank_run.cache_clear()
    b = _bank_run("big", True, "reference", "mse")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[3] + list(a[2]), b[3] + list(b[2])))


def _synthetic_rollout(T, E, N, S, seed):
    g = torch.Generator().manual_seed(seed)
    return {"states": (torch.randn(T, E, N, S, generator=g) * 1.5).cuda(),
            "actions": torch.randint(0, U.N_A, (T, E, N), generator=g, dtype=torch.int32).cuda(),
            "returns": (torch.randn(T, E, N, generator=g) * 2.0).cuda()}


def _nets(K, n_s, seed):
    torch.manual_seed(seed)
    nets = [ActorCriticNetwork(n_s, U.N_A, 128, 1, state_split=True) for _ in range(K)]
    with torch.no_grad():
        for m in nets:
            m.actor_linear.weight.mul_(3.0)
    return [m.cuda() for m in nets]


def _state_of(learner):
    out = learner.params + learner.targets + learner.state1 + [learner.steps, learner._grad_norm]
    if learner.state2 is not None:
        out = out + learner.state2
    return out


def _member_state(learner, k):
    """Member k's parameters, targets, optimiser state, step and norm."""
    stacked = learner.params + learner.targets + learner.state1 + ([] if learner.state2 is None else learner.state2)
    return [t[k] for t in stacked] + [learner.steps[k], learner._grad_norm[k]]


@pytest.mark.parametrize("optimizer_type", ["rmsprop", "adam"])
def test_train_is_graph_capturable(optimizer_type):
    """A torch.cuda.graph capture of train() -- eval, eval, train and opt step per agent step -- replays to the eager bits."""
    K, groups, T, N, S = 3, [3, 0, 5], 4, 2, 30
    learner = SharedBankPPOLearner(_nets(K, S, 11), _lib(), groups, optimizer_type=optimizer_type, target_tau=0.5)
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


def test_the_host_col_start_is_not_read_after_enqueue():
    """Raw eval + train captured with one host table that is overwritten before the replay: the launches carry their own copy."""
    clib, b = _lib(), _batch("mixed", True)
    W = _members(b.K)
    base = _bank_run("mixed", True, "reference", "mse")
    G = [torch.full_like(t, float("nan")) for t in W]
    Ws, Gs = U.struct(W), U.struct(G)
    table = U.c_cols(b.cols)
    loss, sums = torch.full((b.K, 3), float("nan"), device="cuda"), torch.full((b.K, 2), float("nan"), device="cuda")
    value, scratch = torch.full((b.n,), float("nan"), device="cuda"), _scratch(b)
    want_value = torch.full((b.n,), float("nan"), device="cuda")
    assert U.bank_eval(clib, b, Ws, None, want_value) == abi.MM_OK
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = U._stream()
        assert clib.lib.mm_policy_gi_bank_eval(b.obs.data_ptr(), b.obs.stride(0), b.rows, b.row_len, b.n_s, b.act.data_ptr(),
                                               b.act.stride(0), b.valid.data_ptr(), C.byref(Ws), b.K, table, 128, U.N_A, None,
                                               value.data_ptr(), s) == abi.MM_OK
        assert clib.lib.mm_policy_gi_bank_train(
            b.obs.data_ptr(), b.obs.stride(0), b.rows, b.row_len, b.n_s, b.act.data_ptr(), b.act.stride(0), b.ret.data_ptr(),
            b.ret.stride(0), b.old_logp.data_ptr(), b.valid.data_ptr(), C.byref(Ws), b.K, table, 128, U.N_A, 0.2,
            abi.GI_CRITIC_LOSS["mse"], U.FORM["reference"], b.target_value.data_ptr(), C.byref(Gs), loss.data_ptr(), sums.data_ptr(),
            None, None, None, scratch.data_ptr(), scratch.numel(), s) == abi.MM_OK
    for k in range(b.K + 1):
        table[k] = 0
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, base[0]) and torch.equal(sums, base[1])
    assert all(torch.equal(x, y) for x, y in zip(G, base[3]))
    assert torch.equal(value, want_value)


# ---- 6. refused calls between canaries
def test_refused_calls_touch_nothing():
    clib, b = _lib(), _batch("mixed", True)
    W = _members(b.K)
    canary = -12345.0
    G = [torch.full_like(t, canary) for t in W]
    scratch = _scratch(b)
    scratch.fill_(0x5A)
    loss, sums = torch.full((b.K, 3), canary, device="cuda"), torch.full((b.K, 2), canary, device="cuda")
    diag = [torch.full((b.n,), canary, device="cuda") for _ in range(3)]
    Ws, Gs = U.struct(W), U.struct(G)

    def train(**kw):
        a = dict(obs=b.obs.data_ptr(), obs_stride=b.obs.stride(0), n_s=b.n_s, K=b.K, cols=U.c_cols(b.cols), hidden=128, n_a=U.N_A,
                 clip=0.2, critic=0, form=0, value_now=b.target_value.data_ptr(), scratch=scratch.data_ptr(), nbytes=scratch.numel(),
                 old=b.old_logp.data_ptr())
        a.update(kw)
        return clib.lib.mm_policy_gi_bank_train(
            a["obs"], a["obs_stride"], b.rows, b.row_len, a["n_s"], b.act.data_ptr(), b.act.stride(0), b.ret.data_ptr(),
            b.ret.stride(0), a["old"], b.valid.data_ptr(), C.byref(Ws), a["K"], a["cols"], a["hidden"], a["n_a"], a["clip"],
            a["critic"], a["form"], a["value_now"], C.byref(Gs), loss.data_ptr(), sums.data_ptr(), diag[0].data_ptr(),
            diag[1].data_ptr(), diag[2].data_ptr(), a["scratch"], a["nbytes"], U._stream())

    def evaluate(**kw):
        a = dict(obs=b.obs.data_ptr(), n_s=b.n_s, K=b.K, cols=U.c_cols(b.cols), hidden=128, n_a=U.N_A, out=True)
        a.update(kw)
        return clib.lib.mm_policy_gi_bank_eval(a["obs"], b.obs.stride(0), b.rows, b.row_len, a["n_s"], b.act.data_ptr(), b.act.stride(0),
                                               b.valid.data_ptr(), C.byref(Ws), a["K"], a["cols"], a["hidden"], a["n_a"],
                                               diag[0].data_ptr() if a["out"] else None, diag[1].data_ptr() if a["out"] else None,
                                               U._stream())

    refused = [dict(obs=None), dict(obs_stride=b.n_s - 1), dict(n_s=24), dict(n_s=33), dict(K=0), dict(K=3), dict(cols=None),
               dict(cols=U.c_cols((0, 0, 5, 6, 22))), dict(cols=U.c_cols((0, 7, 5, 6, 23))), dict(hidden=512), dict(n_a=0), dict(n_a=9),
               dict(clip=-0.1), dict(critic=2), dict(form=2), dict(value_now=None), dict(form=1), dict(old=None), dict(scratch=None),
               dict(scratch=scratch.data_ptr() + 4), dict(nbytes=scratch.numel() - 1)]
    for change in refused:
        assert train(**change) == abi.MM_ERR_INVALID_ARG, change
    for change in (dict(obs=None), dict(n_s=24), dict(K=0), dict(cols=None), dict(cols=U.c_cols((0, 0, 5, 6, 22))), dict(hidden=512),
                   dict(n_a=9), dict(out=False)):
        assert evaluate(**change) == abi.MM_ERR_INVALID_ARG, change
    torch.cuda.synchronize()
    for t in G + [loss, sums] + diag:
        assert bool((t == canary).all())
    assert bool((scratch == 0x5A).all())


# ---- 7. the learner, no env
CASES = [(7, (2, 0, 3), 3), (13, (5, 1, 0, 7), 4)]


def _valid_of(T, E, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(T, E, N, generator=g) < 0.7).to(torch.uint8).cuda()


def _episodes(K):
    return [5, 0, 10, 3][:K]  # members 0 and 2 blend, 1 and 3 do not


@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("optimizer_type", ["rmsprop", "adam"])
@pytest.mark.parametrize("case", CASES)
def test_learner_flat_equals_shared_ppo_learner_per_member(case, optimizer_type, with_valid):
    """Form "flat", two train() calls: every member's parameters, targets and optimiser state are those of a
    SharedPPOLearner(fused_step=True) on its slice, bit for bit; the optimiser state moves to that learner and back."""
    T, groups, N = case
    K, E, S, clib = len(groups), sum(groups), 30, _lib()
    nets = _nets(K, S, 21)
    first = [copy.deepcopy(m) for m in nets]
    kw = dict(optimizer_type=optimizer_type, target_tau=0.5, critic_loss="huber")
    bank = SharedBankPPOLearner(nets, clib, groups, **kw)
    for k, m in enumerate(nets):  # the modules' parameters and gradients alias the stacks
        for i, p in enumerate(_params(m)):
            assert p.data_ptr() == bank.params[i][k].data_ptr() and p.grad.data_ptr() == bank.grads[i][k].data_ptr()
    solo = [SharedPPOLearner(copy.deepcopy(m), clib, fused_step=True, **kw) for m in first]
    eps = _episodes(K)
    for rnd in range(2):
        batch = _synthetic_rollout(T, E, N, S, 30 + rnd)
        valid = _valid_of(T, E, N, 40 + rnd) if with_valid else None
        losses = bank.train(batch, n_episodes=eps, form="flat", valid=valid)
        assert len(losses) == 1 and tuple(losses[0].shape) == (K, 3)
        for k in range(K):
            sl = slice(bank.env_start[k], bank.env_start[k + 1])
            part = {key: batch[key][:, sl] for key in batch}
            want = solo[k].train(part, n_episodes=eps[k], form="flat", valid=None if valid is None else valid[:, sl])
            if groups[k]:
                assert torch.equal(losses[0][k], want[0]), (k, losses[0][k], want[0])
            f = solo[k]._fused[0]
            mine = _member_state(bank, k)
            theirs = (_params(solo[k].policy) + _params(solo[k].policy_target) + f.state1 + ([] if f.state2 is None else f.state2)
                      + [f.step[0], solo[k]._grad_norm[0]])
            assert len(mine) == len(theirs) and all(torch.equal(x, y.detach()) for x, y in zip(mine, theirs)), (rnd, k)
    assert bank.steps.tolist() == [2] * K and tuple(bank.last_grad_norm().shape) == (K,)
    for k in range(K):  # members 0 and 2 blended their targets, the others did not (an empty group's parameters never move)
        moved = not torch.equal(bank.targets[6][k], first[k].fc2.weight.detach())
        assert moved == (eps[k] % 5 == 0 and eps[k] > 0 and groups[k] > 0), k
    # a member's optimiser state moves to a SharedPPOLearner and back
    sd = bank.optimizer_state_dict(0)
    solo[1].load_optimizer_state_dict(sd)
    bank.load_optimizer_state_dict(K - 1, solo[1].optimizer_state_dict())
    assert int(bank.steps[K - 1]) == int(bank.steps[0]) == 2
    assert all(torch.equal(t[K - 1], t[0]) for t in bank.state1 + (bank.state2 or []))


@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_learner_reference_equals_one_member_learners(case, with_valid):
    """Form "reference", two train() calls: the K-member learner equals K one-member SharedBankPPOLearners on their slices, bit
    for bit.  (Against SharedPPOLearner the S+ / S- rounding differs: test_adv_sums_within_one_ulp_of_float64 bounds it.)"""
    T, groups, N = case
    K, E, S, clib = len(groups), sum(groups), 30, _lib()
    nets = _nets(K, S, 23)
    kw = dict(optimizer_type="adam", target_tau=0.5)
    solo = [SharedBankPPOLearner([copy.deepcopy(m)], clib, [groups[k]], **kw) for k, m in enumerate(nets)]
    bank = SharedBankPPOLearner(nets, clib, groups, **kw)
    eps = _episodes(K)
    for rnd in range(2):
        batch = _synthetic_rollout(T, E, N, S, 50 + rnd)
        valid = _valid_of(T, E, N, 60 + rnd) if with_valid else None
        losses = bank.train(batch, n_episodes=eps, form="reference", valid=valid)
        assert len(losses) == N and all(tuple(l.shape) == (K, 3) for l in losses)
        assert all(bool(torch.isfinite(l).all()) for l in losses)
        for k in range(K):
            sl = slice(bank.env_start[k], bank.env_start[k + 1])
            part = {key: batch[key][:, sl] for key in batch}
            want = solo[k].train(part, n_episodes=eps[k], form="reference", valid=None if valid is None else valid[:, sl])
            assert all(torch.equal(l[k], w[0]) for l, w in zip(losses, want)), k
            assert all(torch.equal(x, y) for x, y in zip(_member_state(bank, k), _member_state(solo[k], 0))), (rnd, k)
    assert bank.steps.tolist() == [2 * N] * K


def test_learner_refuses_a_batch_that_does_not_match_group_envs():
    learner = SharedBankPPOLearner(_nets(2, 30, 2), _lib(), [3, 5])
    with pytest.raises(ValueError, match="do not match the batch"):
        learner.train(_synthetic_rollout(2, 7, 2, 30, 1))
    with pytest.raises(ValueError, match="do not match the batch"):
        learner.evaluate(torch.zeros(16, 30, device="cuda"), torch.zeros(16, dtype=torch.int32, device="cuda"), 2, col_start=[0, 3, 9])
    with pytest.raises(ValueError, match="one int per member"):
        learner.train(_synthetic_rollout(2, 8, 2, 30, 1), n_episodes=[5, 5, 5])
    with pytest.raises(ValueError, match="one non-negative env count per member"):
        SharedBankPPOLearner(_nets(2, 30, 2), _lib(), [8])
    with pytest.raises(ValueError, match="form must be"):
        learner.train(_synthetic_rollout(2, 8, 2, 30, 1), form="literal")


# ---- 8. rollout -> train end to end
@pytest.mark.parametrize("form", ["reference", "flat"])
def test_rollout_to_train_end_to_end(form):
    """v1 MASS, exact QP, E = 16, N = 4, T = 4, K = 2 shared members: interact() -> train(); losses and parameters are finite, the
    parameters moved, and after the next interact() the rollout's stack is the learner's."""
    from marl_mass_amd import VecMergeEnv
    E, N, T, groups = 16, 4, 4, [8, 8]
    nets = _nets(2, 30, 31)
    first = [copy.deepcopy(m) for m in nets]
    env = VecMergeEnv(E, N, config={"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}, cbf_eta=0.03125, qp_solver="exact", cbf_tau=0.5,
                      seed=9, auto_reset=True)
    ro = DeviceRollout(env, nets, roll_out_n_steps=T, sample_seed=4, group_envs=groups)
    assert ro.fused_policy and ro.shared_bank is not None and ro.shared_bank.K == 2
    learner = SharedBankPPOLearner(nets, _lib(), groups, target_tau=0.5)
    out = ro.interact()
    losses = learner.train(out, n_episodes=[5, 0], form=form)
    assert len(losses) == (N if form == "reference" else 1)
    assert all(bool(torch.isfinite(l).all()) for l in losses)
    assert all(bool(torch.isfinite(t).all()) for t in learner.params)
    for k in range(2):
        assert not torch.equal(learner.params[6][k], first[k].fc2.weight.detach())
    ro.interact()
    assert all(torch.equal(t, s) for t, s in zip(ro.shared_bank.tensors, learner.params))
    env.poll_errors()
    env.close()
