"""mm_policy_train / mm_policy_eval (include/mm_policy_train.h) and PPOLearner on the MI355X: both losses and the twelve
gradients against torch.autograd in float64, on synthetic batches and on the batches the reference's MAPPO.train() ran on
(tests/golden/mappo_train_*.npz); the optimiser steps and the soft update against the reference's recorded parameters;
determinism, graph capture, degenerate inputs; DeviceRollout.interact() -> train() end to end.

The tolerance is measured, not fixed (the rule of tests/test_policy_gi_train_gpu.py): in each comparison the float32
torch.autograd gradient is computed too, e32 = max-abs(grad_f32_torch - grad_f64) per tensor, and the kernel's max-abs error
must be <= 4 e32 + 1e-6 max-abs(grad_f64).  Both are float32 sums of n terms in a different order (split-K partial blocks
here, rocBLAS there) and either may be the luckier one, hence the margin of 4; a layout or masking bug shows as an error of
the gradient's own size."""
import copy
import ctypes
import json
import os

import pytest
import torch

from marl_mass_amd import _cabi as abi
from marl_mass_amd.learner import PPOLearner, _mlp_struct
from marl_mass_amd.rollout import ActorNetwork, CriticNetwork, DeviceRollout
from policy_train_util import (FIXTURES, GRAD_NAMES, NAMES, RUNS, fixture_nets, load_fixture, loss_and_grads, one_hot,
                               pre_step_prefix, sums_of)

pytestmark = pytest.mark.gpu

ERRORS = {}  # case -> measured figures; _dump_errors writes their summary when the module is done
LR, RMS_EPS = 1e-4, 1e-8
LOSS_AND_GRADS = ["loss"] + GRAD_NAMES


@pytest.fixture(scope="module", autouse=True)
def _dump_errors(tmp_path_factory):
    """Writes the summary of the measured figures when the module is done: to $MM_GRAD_ERROR_JSON when set (that is how
    profiles/policy_train/grad_error.json is regenerated), else to pytest's temporary directory -- a test run leaves the
    checkout as it found it."""
    yield
    path = os.environ.get("MM_GRAD_ERROR_JSON") or str(tmp_path_factory.mktemp("policy_train") / "grad_error.json")
    with open(path, "w") as f:  # one case per line, three significant digits
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(_rounded(ERRORS[k]), sort_keys=True))
                                   for k in sorted(ERRORS)) + "\n}\n")
    print("measured figures: %s" % path)


def _rounded(x):
    """What is written per case: the tensor closest to its bound -- its name, e32, the kernel's error (or the parameter
    difference of an optimiser-step comparison) and that error as a fraction of the bound."""
    if isinstance(x, dict) and x and all(isinstance(v, dict) for v in x.values()):
        key = "kernel_err" if "kernel_err" in next(iter(x.values())) else "param_diff"
        frac = lambda k: x[k][key] / x[k]["bound"] if x[k]["bound"] > 0 else (0.0 if x[k][key] == 0 else float("inf"))  # noqa: E731
        name = max(x, key=frac)  # (a bound of 0: a gradient that is identically zero, e.g. the actor head with one action)
        return {"worst": name, "of_bound": float("%.3g" % frac(name)), "e32": _rounded(x[name]["e32"]),
                key: _rounded(x[name][key])}
    if isinstance(x, dict):
        return {k: _rounded(v) for k, v in x.items()}
    return float("%.3g" % x) if isinstance(x, float) else x


def _lib():
    from marl_mass_amd import hip_library
    return hip_library()


def _nets(n_s, n_a=5, seed=5):
    """(actor, critic) with the scales of tests/test_policy_gi_train_gpu.py: asymmetric, non-trivial in every layer."""
    torch.manual_seed(seed)
    actor, critic = ActorNetwork(n_s, 128, n_a), CriticNetwork(n_s, n_a, 128, 1)
    with torch.no_grad():  # (on the host: the networks, like the batches below, do not depend on the device's generator)
        for m in (actor.fc1, actor.fc2, critic.fc1, critic.fc2):
            m.bias.uniform_(-0.5, 0.5)
        actor.fc3.bias.uniform_(-1, 1); actor.fc3.weight.mul_(3.0)
        critic.fc3.bias.fill_(0.5); critic.fc3.weight.mul_(2.0)
        critic.fc2.weight[:, 128:].mul_(3.0)  # the one-hot columns matter as much as a hidden unit
    return actor.cuda(), critic.cuda()


def _learner(actor, critic, **kw):
    """A PPOLearner whose targets have moved away from the networks (as after a few optimiser steps)."""
    learner = PPOLearner(actor, critic, _lib(), **kw)
    g = torch.Generator().manual_seed(99)
    with torch.no_grad():
        for p in list(learner.actor_target.parameters()) + list(learner.critic_target.parameters()):
            p.add_(0.01 * torch.randn(p.shape, generator=g).cuda())
    return learner


def _grads_of(actor, critic):
    out = []
    for net in (actor, critic):
        named = dict(net.named_parameters())
        out += [named[k].grad.detach().clone() for k in NAMES]
    return out


def _poison(actor, critic):
    for p in list(actor.parameters()) + list(critic.parameters()):
        p.grad.fill_(float("nan"))  # written, not accumulated


def _compare(case, kernel, f32, f64):
    """kernel / f32 / f64: (loss [2], [12 gradients]).  Prints, records and asserts the module docstring's rule."""
    rec = {}
    bad = []
    rows = [("loss", kernel[0].double(), f32[0].double(), f64[0])] + [
        (k, kernel[1][i].double(), f32[1][i].double(), f64[1][i]) for i, k in enumerate(GRAD_NAMES)]
    for name, gk, g32, g64 in rows:
        e32 = float((g32 - g64).abs().max())
        err = float((gk - g64).abs().max())
        mx = float(g64.abs().max())
        bound = 4.0 * e32 + 1e-6 * mx
        rec[name] = {"e32": e32, "kernel_err": err, "max_abs": mx, "bound": bound}
        print("%-40s %-22s e32 %.3e kernel %.3e max %.3e bound %.3e" % (case, name, e32, err, mx, bound))
        if not err <= bound:
            bad.append((name, err, bound))
    ERRORS[case] = rec
    assert not bad, (case, bad)
    return rec


KNIFE = 2e-5
MAX_REDRAW_SHARE = 0.03


@torch.no_grad()
def _knife_edges(actor64, critic64, obs64, act):
    """Samples with a pre-activation of any of the FOUR hidden layers (both networks) within KNIFE of zero, float64."""
    za1 = actor64.fc1(obs64)
    za2 = actor64.fc2(torch.relu(za1))
    zc1 = critic64.fc1(obs64)
    zc2 = critic64.fc2(torch.cat([torch.relu(zc1), one_hot(act, critic64.fc2.weight.shape[1] - 128, torch.float64)], 1))
    close = torch.zeros(obs64.shape[0], dtype=torch.bool, device=obs64.device)
    for z in (za1, za2, zc1, zc2):
        close |= z.abs().min(dim=1).values < KNIFE
    return close


def _batch(learner, n, n_s, ratio, strided, with_valid, seed, n_a=5, knife_filter=True):
    """A synthetic batch; returns (obs, actions, returns, old_logp, advantages, valid) with the population checks of the inputs.

    The populations are stratified, not left to chance, so that the checks hold at n = 31 as well as at 524 301: a random
    permutation gives every sample a rank k; the ratio is the k-th point of an even grid over [0.5, 1.6], the return noise
    is negative for even k, the action is (k // 2) % n_a, and the mask drops k % 10 in {2, 5, 8} -- 30 % of the samples, evenly
    over the ratio grid, both signs and every action.  The advantages are what PPOLearner computes them from: the returns
    minus the CRITIC TARGET's value (mm_policy_eval), float32; the same tensor goes to the kernel and to both torch runs.

    The knife-edge filter (below) may redraw at most MAX_REDRAW_SHARE = 3 % of a batch.  About 1.3 % of the samples qualify
    (0.65 % per network), so the large batches sit at 0.7 .. 2.1 %; at n = 31 a single sample is 3.2 %, and the four batches of
    that size used here (n_s 25 / 30, contiguous / strided, seed 1 + n + n_s) need no redraw at all -- with a host generator
    that is a fixed property of the inputs, asserted like every other population."""
    actor, critic = learner.actor, learner.critic
    # every draw comes from a host generator: which samples the knife-edge filter below redraws is then a property of
    # (seed, n, n_s, n_a, strided) alone, the same on every machine
    g = torch.Generator().manual_seed(seed)
    k = torch.randperm(n, generator=g).cuda()
    stratified = ((k // 2) % n_a).to(torch.int32)
    if strided:  # states[:, agent_id, :] of a [B, N, S] tensor, actions / returns[:, agent_id] of [B, N]
        obs = (torch.randn(n, 3, n_s, generator=g) * 1.5).cuda()[:, 1, :]
        act = torch.randint(0, n_a, (n, 3), generator=g, dtype=torch.int32).cuda()
        act[:, 1] = stratified
        act = act[:, 1]
        noise = torch.randn(n, 3, generator=g).cuda()[:, 1]
        assert not obs.is_contiguous() and act.stride(0) == 3
    else:
        obs = (torch.randn(n, n_s, generator=g) * 1.5).cuda()
        act = stratified.contiguous()
        noise = torch.randn(n, generator=g).cuda()
    noise = noise.abs() * torch.where(k % 2 == 0, -1.0, 1.0)
    a64, c64 = copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
    # A ReLU whose pre-activation is within float32 rounding of zero is open in one float32 implementation and shut in
    # another: each such unit moves a gradient by O(1 / B), float32 torch against float64 as much as the kernel.  Like r on a
    # clip edge these points are not differentiable and are not tested: samples with a float64 pre-activation of any of the
    # four hidden layers closer to zero than KNIFE are redrawn (decided on the inputs with the float64 networks, never on
    # the kernel).  The filter may touch at most MAX_REDRAW_SHARE of a batch: it removes a measure-zero set, not a population.
    redrawn = 0
    for _ in range(20 if knife_filter else 0):
        close = _knife_edges(a64, c64, obs.double(), act)
        if not bool(close.any()):
            break
        redrawn += int(close.sum())
        obs[close] = (torch.randn(int(close.sum()), n_s, generator=g) * 1.5).cuda()
    if knife_filter:
        assert not bool(_knife_edges(a64, c64, obs.double(), act).any())
        share = redrawn / float(n)
        ERRORS.setdefault("knife_redraw_share", {})["n%d_s%d_a%d_%s" % (n, n_s, n_a, "strided" if strided else "contig")] = share
        assert share <= MAX_REDRAW_SHARE, (n, redrawn)
    oh = one_hot(act, n_a, torch.float64)
    with torch.no_grad():
        logp = a64(obs.double()).gather(1, act.long().unsqueeze(1)).squeeze(1)
        value = c64(obs.double(), oh).squeeze(1)
        tvalue = copy.deepcopy(learner.critic_target).double()(obs.double(), oh).squeeze(1)
    # |value - return| on both sides of the huber knee.  The offset keeps mean(value - return), the critic bias's one-element
    # gradient, from cancelling to ~1e-5 of its terms: there the 1e-6 max-abs floor vanishes and the test would compare two
    # single random rounding draws.
    ret64 = value + 1.5 * noise.double() + 0.3
    if strided:
        ret = torch.zeros(n, 3, device="cuda")
        ret[:, 1] = ret64.float()
        ret = ret[:, 1]
    else:
        ret = ret64.float()
    if ratio == "one":
        old = logp.float()  # (the kernel's own float32 log-probabilities differ in the last bits: r = 1 +- 1e-6, inside the band)
    else:
        u = 0.5 + 1.1 * (k.double() + 0.5) / n
        # r exactly on 1 +- clip has measure zero and is not tested: move the few samples within 1e-3 of an edge off it, so
        # float32 and float64 put every sample on the same side
        near = ((u - 0.8).abs() < 1e-3) | ((u - 1.2).abs() < 1e-3)
        u = torch.where(near, u + 2.5e-3, u)
        old = (logp - torch.log(u)).float()
    valid = None
    if with_valid:
        valid = (~torch.isin(k % 10, torch.tensor([2, 5, 8], device="cuda"))).to(torch.uint8)
    adv = learner.advantages(obs, act, ret, valid)
    # population of the INPUTS (float64 networks), asserted for every n: both clip sides and the band, both signs of advantage,
    # >= 10 % of the valid samples each and never fewer than 3 samples; both sides of the huber knee; every action
    keep = slice(None) if valid is None else valid.bool()
    r = torch.exp(logp - old.double())[keep]
    adv64 = (ret.double() - tvalue)[keep]
    assert float((adv.double()[keep] - adv64).abs().max()) <= 1e-4  # the float32 advantages are those of the critic target
    d = (value - ret.double()).abs()[keep]
    sets = [adv64 > 0, adv64 < 0, d < 1.0, d > 1.0]
    if ratio == "one":
        assert float((r - 1).abs().max()) < 1e-5
    else:
        sets += [r < 0.8, r > 1.2, (r >= 0.8) & (r <= 1.2)]
        assert float(((r - 0.8).abs() < 1e-4).sum() + ((r - 1.2).abs() < 1e-4).sum()) == 0  # nobody on a clip edge
    for m in sets:
        assert float(m.double().mean()) >= 0.10 and int(m.sum()) >= 3, (n, int(m.sum()), int(m.numel()))
    counts = torch.bincount(act[keep].long(), minlength=n_a)
    assert int(counts.numel()) == n_a and float(counts.min()) >= float(counts.sum()) / (2 * n_a)  # every one-hot column is hit
    return obs, act, ret, old, adv, valid


def _torch_sides(learner, obs, act, ret, old, adv, valid, form, sums, critic_loss, clip=0.2):
    actor, critic = learner.actor, learner.critic
    a32, c32, a64, c64 = copy.deepcopy(actor), copy.deepcopy(critic), copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
    f32 = loss_and_grads(a32, c32, obs, act, ret, old, clip, critic_loss, form, advantages=adv, adv_sums=sums, valid=valid)
    f64 = loss_and_grads(a64, c64, obs.double(), act, ret.double(), old.double(), clip, critic_loss, form, advantages=adv.double(),
                         adv_sums=None if sums is None else sums.double(), valid=valid)
    return f32, f64


def _launch(learner, obs, act, ret, old, adv, valid, form, diagnostics=False):
    """(sums, result of loss_and_grad): the same float32 (S+, S-) goes to the kernel and, as a constant, to both torch runs."""
    sums = sums_of(adv) if form == "reference" else None
    out = learner.loss_and_grad(obs, act, ret, old, valid=valid, adv_sums=sums, advantages=None if sums is not None else adv,
                                diagnostics=diagnostics)
    return sums, out


@pytest.mark.parametrize("ratio", ["one", "spread"])
@pytest.mark.parametrize("strided", [False, True], ids=["contig", "strided"])
@pytest.mark.parametrize("with_valid", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("critic_loss", ["mse", "huber"])
@pytest.mark.parametrize("form", ["reference", "flat"])
@pytest.mark.parametrize("n_s", [25, 30])
@pytest.mark.parametrize("n", [31, 1000, 524301])
def test_gradient_matches_autograd(n, n_s, form, critic_loss, with_valid, strided, ratio):
    actor, critic = _nets(n_s)
    learner = _learner(actor, critic, critic_loss=critic_loss)
    obs, act, ret, old, adv, valid = _batch(learner, n, n_s, ratio, strided, with_valid, seed=1 + n + n_s)
    _poison(actor, critic)
    sums, (loss, (lp, v, r)) = _launch(learner, obs, act, ret, old, adv, valid, form, diagnostics=True)
    kernel = (loss.clone(), _grads_of(actor, critic))
    f32, f64 = _torch_sides(learner, obs, act, ret, old, adv, valid, form, sums, critic_loss)
    case = "n%d_s%d_%s_%s_%s_%s_%s" % (n, n_s, form, critic_loss, "valid" if with_valid else "all",
                                     "strided" if strided else "contig", ratio)
    _compare(case, kernel, f32, f64)
    # diagnostics: log-probability, value and ratio per sample (zeros in masked slots)
    with torch.no_grad():
        lp64 = copy.deepcopy(actor).double()(obs.double()).gather(1, act.long().unsqueeze(1)).squeeze(1)
        v64 = copy.deepcopy(critic).double()(obs.double(), one_hot(act, 5, torch.float64)).squeeze(1)
    keep = torch.ones(n, dtype=torch.bool, device="cuda") if valid is None else valid.bool()
    assert float((lp.double() - lp64)[keep].abs().max()) <= 2e-5
    assert bool(((v.double() - v64).abs() <= 1e-5 * v64.abs().clamp(min=1.0))[keep].all())
    assert float((r.double() - torch.exp(lp64 - old.double()))[keep].abs().max()) <= 1e-4
    if valid is not None:
        assert float(lp[~keep].abs().max()) == 0.0 and float(r[~keep].abs().max()) == 0.0 and float(v[~keep].abs().max()) == 0.0


@pytest.mark.parametrize("form", ["reference", "flat"])
@pytest.mark.parametrize("n_a", [1, 8])
def test_action_counts(n_a, form):
    """The ends of the n_a range (every other case has 5 actions), masked and strided: the critic's fc2 is [128][129] and
    [128][136], every one-hot column populated (asserted in _batch)."""
    n, n_s = 1000, 30
    actor, critic = _nets(n_s, n_a=n_a)
    learner = _learner(actor, critic, critic_loss="huber")
    obs, act, ret, old, adv, valid = _batch(learner, n, n_s, "spread", True, True, seed=11 + n_a, n_a=n_a)
    _poison(actor, critic)
    sums, loss = _launch(learner, obs, act, ret, old, adv, valid, form)
    kernel = (loss.clone(), _grads_of(actor, critic))
    f32, f64 = _torch_sides(learner, obs, act, ret, old, adv, valid, form, sums, "huber")
    _compare("n_a%d_%s" % (n_a, form), kernel, f32, f64)


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_one_network_alone(which):
    """Either network may be left out: the other's gradient and loss are the ones of the joint call, bit for bit, and the
    omitted network's .grad is not touched."""
    n, n_s = 1000, 30
    actor, critic = _nets(n_s)
    learner = _learner(actor, critic)
    obs, act, ret, old, adv, valid = _batch(learner, n, n_s, "spread", True, True, seed=21)
    learner.loss_and_grad(obs, act, ret, old, valid=valid, advantages=adv)
    both = _grads_of(actor, critic)
    _poison(actor, critic)
    loss = learner.loss_and_grad(obs, act, ret, old, valid=valid, advantages=adv, networks=which)
    alone = _grads_of(actor, critic)
    mine = slice(0, 6) if which == "actor" else slice(6, 12)
    other = slice(6, 12) if which == "actor" else slice(0, 6)
    assert all(torch.equal(x, y) for x, y in zip(both[mine], alone[mine]))
    assert all(bool(torch.isnan(x).all()) for x in alone[other])
    assert float(loss[1 if which == "actor" else 0]) == 0.0 and float(loss[0 if which == "actor" else 1]) != 0.0


def test_unfiltered_batch_figures():
    """What the knife-edge filter of _batch removes, in figures (profiles/policy_train/grad_error.json, "unfiltered_*"): the
    largest batch WITHOUT the filter.  Each ReLU within float32 rounding of zero that one implementation opens and the other
    shuts moves a gradient element by one sample's contribution, O(1 / B) of an O(1) term, so here the float32 torch error
    and the kernel's error are both set by a handful of such units and either can exceed 4 x the other.  Asserted: the
    kernel's error stays of that size -- <= 1e-3 of each tensor's max-abs (reasoning: a flipped unit contributes at most
    |dz| |x| / B ~ 10 / 524 301 = 2e-5 against gradients of 1e-3 .. 1e-2, a few units per tensor; a layout or masking bug
    gives an error of the tensor's own size).  The 4 e32 rule is asserted on the filtered batches and on the fixtures."""
    n, n_s = 524301, 25
    actor, critic = _nets(n_s)
    learner = _learner(actor, critic, critic_loss="huber")
    obs, act, ret, old, adv, valid = _batch(learner, n, n_s, "spread", True, False, seed=1 + n + n_s, knife_filter=False)
    loss = learner.loss_and_grad(obs, act, ret, old, advantages=adv)
    kernel = (loss.clone(), _grads_of(actor, critic))
    f32, f64 = _torch_sides(learner, obs, act, ret, old, adv, None, "flat", None, "huber")
    close = _knife_edges(copy.deepcopy(actor).double(), copy.deepcopy(critic).double(), obs.double(), act)
    rec = {"samples_within_KNIFE": int(close.sum()), "share_within_KNIFE": float(close.double().mean())}
    for name, gk, g32, g64 in zip(LOSS_AND_GRADS, [kernel[0]] + kernel[1], [f32[0]] + f32[1], [f64[0]] + f64[1]):
        e32, err, mx = (float((g32.double() - g64).abs().max()), float((gk.double() - g64).abs().max()), float(g64.abs().max()))
        rec[name] = "e32 %.3g kernel %.3g max_abs %.3g" % (e32, err, mx)
        print("unfiltered %-22s %s" % (name, rec[name]))
        assert err <= 1e-3 * mx, (name, err, mx)
    ERRORS["unfiltered_n524301_s25_flat_huber_all_strided_spread"] = rec


@pytest.mark.parametrize("strided", [False, True], ids=["contig", "strided"])
@pytest.mark.parametrize("with_valid", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("which", ["actor", "critic", "both"])
@pytest.mark.parametrize("n,n_s,n_a", [(31, 25, 5), (70001, 30, 5), (1000, 32, 8), (1000, 30, 1)])
def test_eval_matches_the_float64_modules(n, n_s, n_a, which, with_valid, strided):
    """mm_policy_eval: the log-probability of the taken action within 2e-5 absolute, the value within 1e-5 relative (floor 1)
    of the float64 modules -- the bounds of the GI diagnostics -- and zeros in masked slots."""
    actor, critic = _nets(n_s, n_a=n_a, seed=8)
    learner = PPOLearner(actor, critic, _lib())
    g = torch.Generator(device="cuda").manual_seed(n + n_s)
    if strided:
        obs = (torch.randn(n, 3, n_s, device="cuda", generator=g) * 1.5)[:, 2, :]
        act = torch.randint(0, n_a, (n, 3), device="cuda", generator=g, dtype=torch.int32)[:, 2]
    else:
        obs = torch.randn(n, n_s, device="cuda", generator=g) * 1.5
        act = torch.randint(0, n_a, (n,), device="cuda", generator=g, dtype=torch.int32)
    valid = (torch.rand(n, device="cuda", generator=g) > 0.3).to(torch.uint8) if with_valid else None
    keep = torch.ones(n, dtype=torch.bool, device="cuda") if valid is None else valid.bool()
    lp, v = learner.evaluate(obs, act, actor=actor if which != "critic" else None, critic=critic if which != "actor" else None,
                             valid=valid)
    assert (lp is None) == (which == "critic") and (v is None) == (which == "actor")
    with torch.no_grad():
        lp64 = copy.deepcopy(actor).double()(obs.double()).gather(1, act.long().unsqueeze(1)).squeeze(1)
        v64 = copy.deepcopy(critic).double()(obs.double(), one_hot(act, n_a, torch.float64)).squeeze(1)
    if lp is not None:
        err = float((lp.double() - lp64)[keep].abs().max())
        assert err <= 2e-5, err
        assert valid is None or float(lp[~keep].abs().max()) == 0.0
    if v is not None:
        assert bool(((v.double() - v64).abs() <= 1e-5 * v64.abs().clamp(min=1.0))[keep].all())
        assert valid is None or float(v[~keep].abs().max()) == 0.0
    # the learner's wrappers are that call on the targets
    if which == "both" and not with_valid:
        assert torch.equal(learner.old_log_probs(obs, act), lp)  # fresh targets == the networks
        ret = torch.randn(n, device="cuda", generator=g)
        assert torch.equal(learner.advantages(obs, act, ret), ret - v)
        assert torch.equal(learner.advantage_sums(obs, act, ret), sums_of(ret - v))


def _fixture_step_inputs(z, a, device="cuda"):
    obs = torch.tensor(z["states"], device=device)[:, a, :]  # strided views, as train() takes them
    act = torch.tensor(z["actions"], device=device)[:, a]
    ret = torch.tensor(z["returns"], device=device)[:, a]
    return obs, act, ret


def _fixture_learner(z, meta, prefix, **kw):
    actor, critic = fixture_nets(z, meta, prefix, device="cuda")
    learner = PPOLearner(actor, critic, _lib(), critic_loss=meta["critic_loss"], clip_param=meta["clip_param"], **kw)
    ta, tc = fixture_nets(z, meta, "tp_", device="cuda")
    learner.actor_target.load_state_dict(ta.state_dict())
    learner.critic_target.load_state_dict(tc.state_dict())
    return learner


@pytest.mark.parametrize("run,t", FIXTURES)
def test_reference_fixture_gradients(run, t):
    """Losses and pre-clip gradients of every agent step the reference recorded: the kernel against float64 autograd of the
    LITERAL [B, B] expression (same rule), and against the recorded float32 numbers within that bound plus the recorded
    run's own distance from float64 (triangle inequality)."""
    z, meta = load_fixture(run, t)
    for a in range(meta["n_agents"]):
        learner = _fixture_learner(z, meta, pre_step_prefix(a))
        obs, act, ret = _fixture_step_inputs(z, a)
        old = learner.old_log_probs(obs, act)
        adv = learner.advantages(obs, act, ret)
        loss = learner.loss_and_grad(obs, act, ret, old, adv_sums=sums_of(adv))
        kernel = (loss.clone(), _grads_of(learner.actor, learner.critic))
        f32, f64 = _torch_sides(learner, obs, act, ret, old, adv, None, "literal", None, meta["critic_loss"], meta["clip_param"])
        rec = _compare("fixture_%s_t%d_a%d" % (run, t, a), kernel, f32, f64)
        recorded = [torch.tensor(z["a%d_losses" % a], device="cuda")] + [torch.tensor(z["a%d_g_%s" % (a, k)], device="cuda")
                                                                        for k in GRAD_NAMES]
        for name, gk, gr, g64 in zip(LOSS_AND_GRADS, [kernel[0]] + kernel[1], recorded, [f64[0]] + f64[1]):
            slack = float((gr.double() - g64).abs().max())
            assert float((gk.double() - gr.double()).abs().max()) <= rec[name]["bound"] + slack, (a, name)


@pytest.mark.parametrize("run", RUNS)
def test_learner_reproduces_the_recorded_optimiser_steps(run):
    """PPOLearner.train(form="reference") from the recorded initial state, train 0 then train 1 with the same learner (both
    RMSprop states carry over), against the recorded post-step parameters of BOTH networks after every agent step.  RMSprop's
    first step is lr g / (0.1 |g| + eps): an element whose gradient is rounding noise around zero moves by up to
    (lr / eps) dg, so per tensor the bound is (lr / eps) 4 e32 + 1e-7 with e32 the float32 torch error on that tensor (max
    over the agent steps), never the kernel's own.  In the "soft" run both targets after train 1 are the recorded ones."""
    z0, meta0 = load_fixture(run, 0)
    kw = dict(actor_lr=meta0["actor_lr"], critic_lr=meta0["critic_lr"], optimizer_type=meta0["optimizer_type"],
              max_grad_norm=meta0["max_grad_norm"], target_tau=meta0["target_tau"], target_update_steps=meta0["target_update_steps"])
    learner = _fixture_learner(z0, meta0, "p_", **kw)
    whole = _fixture_learner(z0, meta0, "p_", **kw)
    observed = {}
    for t in (0, 1):
        z, meta = load_fixture(run, t)
        N = meta["n_agents"]
        states, actions, returns = (torch.tensor(z[k], device="cuda") for k in ("states", "actions", "returns"))
        e32 = dict.fromkeys(GRAD_NAMES, 0.0)
        for a in range(N):
            # e32 of this step: float32 vs float64 autograd at the RECORDED pre-step parameters and targets
            pre = _fixture_learner(z, meta, pre_step_prefix(a))
            obs, act, ret = _fixture_step_inputs(z, a)
            old, adv = pre.old_log_probs(obs, act), pre.advantages(obs, act, ret)
            f32, f64 = _torch_sides(pre, obs, act, ret, old, adv, None, "literal", None, meta["critic_loss"], meta["clip_param"])
            for k, x, y in zip(GRAD_NAMES, f32[1], f64[1]):
                e32[k] = max(e32[k], float((x.double() - y).abs().max()))
            # one agent step = train() on that agent's column alone; the soft update belongs to the LAST column's call only
            last = a == N - 1
            learner.train(states[:, a:a + 1], actions[:, a:a + 1], returns[:, a:a + 1], n_episodes=meta["n_episodes"] if last else 0)
            named = {"actor." + k: v for k, v in learner.actor.named_parameters()}
            named.update({"critic." + k: v for k, v in learner.critic.named_parameters()})
            for k in GRAD_NAMES:
                diff = float((named[k].detach() - torch.tensor(z["a%d_q_%s" % (a, k)], device="cuda")).abs().max())
                bound = (LR / RMS_EPS) * 4.0 * e32[k] + 1e-7
                observed["t%d_a%d_%s" % (t, a, k)] = {"param_diff": diff, "bound": bound, "e32": e32[k]}
                print("%s t%d a%d %-22s diff %.3e bound %.3e" % (run, t, a, k, diff, bound))
                assert diff <= bound, (t, a, k, diff, bound)
        # the same N steps as ONE train() call: bit-identical to the column-by-column learner, targets included
        whole.train(states, actions, returns, n_episodes=meta["n_episodes"])
        for m1, m2 in ((learner.actor, whole.actor), (learner.critic, whole.critic), (learner.actor_target, whole.actor_target),
                       (learner.critic_target, whole.critic_target)):
            for p, q in zip(m1.parameters(), m2.parameters()):
                assert torch.equal(p, q)
        targets = {"actor." + k: v for k, v in learner.actor_target.named_parameters()}
        targets.update({"critic." + k: v for k, v in learner.critic_target.named_parameters()})
        for k in GRAD_NAMES:
            if meta["soft_update_after_train"]:
                # the blend of the recorded and of this run's final networks: half the parameter bound, plus the blend's rounding
                want = torch.tensor(z["after_tp_" + k], device="cuda")
                bound = meta["target_tau"] * ((LR / RMS_EPS) * 4.0 * e32[k] + 1e-7) + 1e-7
                diff = float((targets[k].detach() - want).abs().max())
                observed["t%d_target_%s" % (t, k)] = {"param_diff": diff, "bound": bound, "e32": e32[k]}
                assert diff <= bound, (t, k, diff, bound)
                assert not torch.equal(targets[k].detach(), torch.tensor(z["tp_" + k], device="cuda"))
            else:  # no soft update: the targets are untouched, bit for bit
                assert torch.equal(targets[k].detach(), torch.tensor(z["tp_" + k], device="cuda"))
    ERRORS["learner_steps_%s" % run] = observed


def test_deterministic_and_graph_capturable():
    n, n_s = 70001, 30
    actor, critic = _nets(n_s)
    learner = _learner(actor, critic)
    obs, act, ret, old, adv, valid = _batch(learner, n, n_s, "spread", True, True, seed=77)
    sums = sums_of(adv)
    runs = []
    for _ in range(2):
        _poison(actor, critic)
        loss = learner.loss_and_grad(obs, act, ret, old, valid=valid, adv_sums=sums)
        runs.append([loss.clone()] + _grads_of(actor, critic))
    for x, y in zip(*runs):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    # capture + replay == eager, bit for bit
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        learner.loss_and_grad(obs, act, ret, old, valid=valid, adv_sums=sums)
        learner.evaluate(obs, act, actor=actor, critic=critic, valid=valid)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager_eval = learner.evaluate(obs, act, actor=actor, critic=critic, valid=valid)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gloss = learner.loss_and_grad(obs, act, ret, old, valid=valid, adv_sums=sums)
        geval = learner.evaluate(obs, act, actor=actor, critic=critic, valid=valid)
    _poison(actor, critic)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(runs[0], [gloss] + _grads_of(actor, critic)):
        assert torch.equal(x, y)
    assert torch.equal(eager_eval[0], geval[0]) and torch.equal(eager_eval[1], geval[1])


def test_degenerate_inputs():
    actor, critic = _nets(30)
    learner = _learner(actor, critic)
    zero = lambda loss: float(loss.abs().max()) == 0.0 and all(float(g.abs().max()) == 0.0 for g in _grads_of(actor, critic))  # noqa: E731
    _poison(actor, critic)
    e = torch.empty(0, 30, device="cuda")
    ei, ef = torch.empty(0, dtype=torch.int32, device="cuda"), torch.empty(0, device="cuda")
    assert zero(learner.loss_and_grad(e, ei, ef, ef, advantages=ef))
    lp, v = learner.evaluate(e, ei, actor=actor, critic=critic)
    assert lp.shape == (0,) and v.shape == (0,)
    obs, act, ret, old, adv, _ = _batch(learner, 500, 30, "spread", False, False, seed=3)
    _poison(actor, critic)
    assert zero(learner.loss_and_grad(obs, act, ret, old, advantages=adv, valid=torch.zeros(500, dtype=torch.uint8, device="cuda")))
    _poison(actor, critic)
    assert zero(learner.loss_and_grad(obs, act, ret, old, adv_sums=sums_of(adv), valid=torch.zeros(500, dtype=torch.uint8, device="cuda")))
    # masked slots may hold anything: NaN observations / returns / advantages and out-of-range actions there change nothing
    valid = torch.ones(500, dtype=torch.uint8, device="cuda")
    valid[::3] = 0
    clean = [learner.loss_and_grad(obs, act, ret, old, advantages=adv, valid=valid).clone()] + _grads_of(actor, critic)
    clean_eval = learner.evaluate(obs, act, actor=actor, critic=critic, valid=valid)
    obs2, act2, ret2, old2, adv2 = obs.clone(), act.clone(), ret.clone(), old.clone(), adv.clone()
    obs2[::3] = float("nan"); ret2[::3] = float("nan"); old2[::3] = float("nan"); adv2[::3] = float("nan"); act2[::3] = 1000
    dirty = [learner.loss_and_grad(obs2, act2, ret2, old2, advantages=adv2, valid=valid).clone()] + _grads_of(actor, critic)
    for x, y in zip(clean, dirty):
        assert torch.equal(x, y)
    for x, y in zip(clean_eval, learner.evaluate(obs2, act2, actor=actor, critic=critic, valid=valid)):
        assert torch.equal(x, y)
    # an out-of-range action in a valid slot is clamped, not read out of bounds
    act3 = act.clone(); act3[0] = 99; act3[1] = -4
    act4 = act.clone(); act4[0] = 4; act4[1] = 0
    a = [learner.loss_and_grad(obs, act3, ret, old, advantages=adv).clone()] + _grads_of(actor, critic)
    b = [learner.loss_and_grad(obs, act4, ret, old, advantages=adv).clone()] + _grads_of(actor, critic)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x, y in zip(learner.evaluate(obs, act3, actor=actor, critic=critic), learner.evaluate(obs, act4, actor=actor, critic=critic)):
        assert torch.equal(x, y)
    torch.cuda.synchronize()
    # invalid arguments -> ValueError through clib.check
    for width in (24, 28, 33):  # not the networks' state size
        with pytest.raises(ValueError):
            learner.loss_and_grad(torch.randn(8, width, device="cuda"), act[:8], ret[:8], old[:8], advantages=adv[:8])
        with pytest.raises(ValueError):
            learner.evaluate(torch.randn(8, width, device="cuda"), act[:8], actor=actor)
    with pytest.raises(ValueError):  # neither form of the advantages
        learner.loss_and_grad(obs, act, ret, old)
    with pytest.raises(ValueError):  # both
        learner.loss_and_grad(obs, act, ret, old, advantages=adv, adv_sums=sums_of(adv))
    with pytest.raises(ValueError):
        learner.loss_and_grad(obs, act, ret, old, advantages=adv, networks="none")
    with pytest.raises(ValueError):
        learner.train(obs.view(100, 5, 30), act.view(100, 5), ret.view(100, 5), form="other")
    small = _learner(actor, critic)
    small._ensure_scratch = lambda n: torch.empty(1024, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        small.loss_and_grad(obs, act, ret, old, advantages=adv)  # scratch too small
    bad = _learner(actor, critic)
    bad.clip_param = -0.1
    with pytest.raises(ValueError):
        bad.loss_and_grad(obs, act, ret, old, advantages=adv)
    clib = _lib()
    Wa, Wc, Ga, Gc = _mlp_struct(actor), _mlp_struct(critic), _mlp_struct(actor, True), _mlp_struct(critic, True)
    l2 = torch.empty(2, device="cuda")
    scratch = learner._ensure_scratch(500)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ref = lambda st: None if st is None else ctypes.byref(st)  # noqa: E731

    def direct(hidden=128, n_a=5, crit=0, wa=Wa, wc=Wc, ga=Ga, gc=Gc, sums=None, advp=adv.data_ptr(), loss=l2.data_ptr(), value=None,
               logp=None, n=500, sc=scratch.data_ptr(), n_s=30, stride=30, clip=0.2):
        clib.check(clib.lib.mm_policy_train(obs.data_ptr(), stride, n, n_s, act.data_ptr(), 1, ret.data_ptr(), 1, old.data_ptr(), None,
                                            ref(wa), ref(wc), hidden, n_a, clip, crit, sums, advp, ref(ga), ref(gc), loss, logp, value,
                                            None, sc, scratch.numel(), stream))

    direct()  # the well-formed call goes through
    probe = torch.empty(500, device="cuda")
    for kw in (dict(n_s=24), dict(n_s=33), dict(stride=29), dict(clip=-0.1), dict(clip=float("nan")), dict(hidden=64), dict(hidden=256), dict(n_a=0), dict(n_a=9), dict(crit=2), dict(wa=None, wc=None, ga=None, gc=None),
               dict(ga=None), dict(wc=None), dict(loss=None), dict(n=-1), dict(sc=None), dict(sc=scratch.data_ptr() + 4),
               dict(wa=None, ga=None, logp=probe.data_ptr()), dict(wc=None, gc=None, value=probe.data_ptr())):
        with pytest.raises(ValueError):
            direct(**kw)
    hollow = abi.MMMlpParams()
    for name in abi.MLP_PARAMS[:-1]:
        setattr(hollow, name, getattr(Wa, name))  # b3 left NULL
    with pytest.raises(ValueError):
        direct(wa=hollow)
    direct(wa=None, ga=None, advp=None)  # critic alone needs no advantages
    with pytest.raises(ValueError):  # a network without its output, an output without its network
        clib.check(clib.lib.mm_policy_eval(obs.data_ptr(), 30, 500, 30, act.data_ptr(), 1, None, ref(Wa), None, 128, 5, None, None, stream))
    with pytest.raises(ValueError):
        clib.check(clib.lib.mm_policy_eval(obs.data_ptr(), 30, 500, 30, act.data_ptr(), 1, None, None, None, 128, 5, probe.data_ptr(),
                                           None, stream))
    torch.cuda.synchronize()


def test_rollout_to_train_end_to_end():
    """DeviceRollout(actor, critic) on 256 envs x 4 -> train(form="flat"), three rounds; round one repeated with the gradients
    taken by float32 torch autograd (same optimisers, same rollout tensors): parameters within the per-tensor RMSprop bound."""
    from marl_mass_amd import VecMergeEnv
    E, N, T = 256, 4, 10
    actor, critic = _nets(30, seed=3)
    start = (copy.deepcopy(actor), copy.deepcopy(critic))
    env = VecMergeEnv(E, N, seed=9, config={"safety_guarantee": "cbf-cav", "HEADWAY_TIME": 0.5}, cbf_eta=0.03125,
                      qp_solver="exact", cbf_tau=0.5, auto_reset=True)
    ro = DeviceRollout(env, actor, critic, roll_out_n_steps=T, sample_seed=4)
    assert not ro.shared and ro.fused_policy
    learner = PPOLearner(actor, critic, env.clib)
    for rnd in range(3):
        out = ro.interact()
        if rnd == 0:
            kept = {k: out[k].clone() for k in ("states", "actions", "returns")}
        losses = learner.train(out, n_episodes=rnd, form="flat")
        assert len(losses) == 1 and bool(torch.isfinite(losses[0]).all())
        assert all(bool(torch.isfinite(p).all()) for p in list(actor.parameters()) + list(critic.parameters()))
    assert all(not torch.equal(p, q) for net, net0 in zip((actor, critic), start) for p, q in zip(net.parameters(), net0.parameters()))
    # round one again: once with the gradients by float32 torch autograd, once by the kernel, from the same parameters
    obs = kept["states"].reshape(-1, 30).float()
    act, ret = kept["actions"].reshape(-1), kept["returns"].reshape(-1).float()
    twin = PPOLearner(copy.deepcopy(start[0]), copy.deepcopy(start[1]), env.clib)
    again = PPOLearner(copy.deepcopy(start[0]), copy.deepcopy(start[1]), env.clib)
    old, adv = twin.old_log_probs(obs, act), twin.advantages(obs, act, ret)
    f32, f64 = _torch_sides(twin, obs, act, ret, old, adv, None, "flat", None, "mse")
    named = {"actor." + k: v for k, v in twin.actor.named_parameters()}
    named.update({"critic." + k: v for k, v in twin.critic.named_parameters()})
    for k, g in zip(GRAD_NAMES, f32[1]):
        named[k].grad = g.clone()
    twin._step()
    again.train(kept, n_episodes=0, form="flat")
    mine = {"actor." + k: v for k, v in again.actor.named_parameters()}
    mine.update({"critic." + k: v for k, v in again.critic.named_parameters()})
    first = {"actor." + k: v for k, v in start[0].named_parameters()}
    first.update({"critic." + k: v for k, v in start[1].named_parameters()})
    observed = {}
    for k, x32, x64 in zip(GRAD_NAMES, f32[1], f64[1]):
        e32 = float((x32.double() - x64).abs().max())
        bound = (LR / RMS_EPS) * 4.0 * e32 + 1e-7
        diff = float((mine[k] - named[k]).detach().abs().max())
        moved = float((named[k] - first[k]).abs().max())
        observed[k] = {"param_diff": diff, "bound": bound, "e32": e32, "step_size": moved}
        print("end-to-end %-22s diff %.3e bound %.3e step %.3e" % (k, diff, bound, moved))
        assert diff <= bound, (k, diff, bound)
    ERRORS["end_to_end_round_one"] = observed
